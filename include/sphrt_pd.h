/*
 * sphrt_pd.h — C ABI of the primal-dual solver's vector side (libsphrt.so, gfx950): the two
 * launches retrieval.primal_dual adds to the operator's own per iteration.  Same conventions as
 * sphrt.h (plain C types, caller-owned device buffers, `stream` a hipStream_t passed as void*,
 * 0 on success, otherwise a message in sphrt_last_error); a header of its own so that the table of
 * sphrt.h's entries, which other files are held to, stays as it is.
 *
 * The problem: min over lower <= x <= upper of F(x) + sum_ax c_ax |D_ax x|_1, F smooth with
 * grad F(x) = g + c_damp x, over a volume of nr x ne x na float64 voxels (row-major, a fastest).
 * D_ax is the forward difference along an axis that has edges (has_ax != 0 and a length > 1),
 * oriented and stored as sphrt_smooth_reg_f64 counts its edges: an edge belongs to its lower
 * voxel, (D_ax x)[i] = x[upper neighbour of i] - x[i]; with wrap_a (and na > 1) the azimuth ring
 * closes by one more edge that belongs to the ring's last voxel and whose upper neighbour is the
 * first (na = 2: two edges between the pair; a ring of one has none).  The dual q is three
 * volumes, q + ax * n for ax = r, e, a (n = nr * ne * na); slots without an edge are never read
 * or written.
 *
 * Launch shape, partition, sphrt_loss_partials and the order of the partial sums are those of
 * the loss entries of sphrt.h: 256 threads, at most 1024 workgroups, grid-stride, element i
 * owned by workgroup (i / 256) mod grid; part_* receive one sum per workgroup.  Every product
 * that feeds a sum is a plain multiply and every update one fma, whatever -ffp-contract says;
 * inf, NaN and denormals are not special-cased (a NaN u or v fails both compares and stays
 * NaN).  `tau` and `sigma` point to one float64 each on the device.  Each entry fails on the
 * host, before any launch and without reading a pointer, on a null buffer, on buffers that
 * overlap, on an axis length < 1, on n >= 2^31, on (primal) a NaN bound or lower >= upper and on
 * (dual) a c_ax that is not finite and >= 0.
 */
#ifndef SPHRT_PD_H
#define SPHRT_PD_H

#include "sphrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/*   gp = fma(c_damp, x[i], g[i])
 *   s  = (D^T q)[i]: from +0.0, over the edges present at i in the order r-, r+, e-, e+, a-, a+:
 *        s = s + q_ax[lower neighbour of i] for the edge arriving at i,
 *        s = s - q_ax[i]                    for the edge leaving i
 *   u  = fma(-*tau, gp + s, x[i]);  x_new[i] = u < lower ? lower : (u > upper ? upper : u)
 *   part_mm: partial sums of (x_new[i] - x[i])^2
 * lower / upper: -inf / +inf for no bound.  x, g, x_new: n elements; q: 3 n.                   */
int sphrt_pd_primal_f64(const double *x, const double *g, const double *q, double *x_new,
                        int nr, int ne, int na, int wrap_a, int has_r, int has_e, int has_a,
                        double c_damp, const double *tau, double lower, double upper,
                        double *part_mm, void *stream);
/*   xb(j) = fma(2, x_new[j], -x_old[j]), formed at i and at its upper neighbours
 *   for ax = r, e, a with an edge leaving i, j its upper neighbour:
 *     v = fma(*sigma, xb(j) - xb(i), q_ax[i])
 *     q_ax[i] = v < -c_ax ? -c_ax : (v > c_ax ? c_ax : v)      (in place: its own thread's slot)
 *   part_qq: partial sums of the voxels' terms, a voxel's term being the axes' (q_ax[i] new -
 *   q_ax[i] old)^2 added in the order r, e, a onto +0.0                                         */
int sphrt_pd_dual_f64(const double *x_new, const double *x_old, double *q,
                      int nr, int ne, int na, int wrap_a, int has_r, int has_e, int has_a,
                      double c_r, double c_e, double c_a, const double *sigma, double *part_qq,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPHRT_PD_H */
