"""Print tests/gd_cases.D_CASE: for every case of the gd matrix, how far the CPU reference moves
when the oracle matrix's row and column sums are formed in the opposite order (coefficients,
reconstructed stack, each loss history), as the literal to paste into tests/gd_cases.py.  CPU only.

    python tools/gd_sensitivity.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np  # noqa: E402

import gd_cases as gc  # noqa: E402


def main():
    print('D_CASE = {')
    for name in gc.NAMES + gc.DECLINED_NAMES:
        d_c, d_y, d_h = gc.sensitivity(name)
        ref = gc.reference(name)
        rel = d_c / float(np.abs(ref.c).max())
        flag = '   # ILL-CONDITIONED: re-seed' if rel > gc.ILL else ''
        hist = ', '.join(f'{d:.3e}' for d in d_h)
        print(f'    {name!r}: ({d_c:.3e}, {d_y:.3e}, [{hist}]),{flag}')
    print('}')


if __name__ == '__main__':
    main()
