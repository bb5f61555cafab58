/*
 * sphrt_iso.h — C ABI of isotropic total variation in the primal-dual solvers (libsphrt.so,
 * gfx950): the two launches retrieval.primal_dual and retrieval.chambolle_pock issue, with a
 * loss.IsoTVRegularizer as their TV term, in place of the two of sphrt_pd.h.  Same conventions as
 * sphrt.h (plain C types, caller-owned device buffers, `stream` a hipStream_t passed as void*,
 * 0 on success, otherwise a message in sphrt_last_error); a header of its own so that the tables
 * of the other headers' entries, which other files are held to, stay as they are.
 *
 * The problem: min over lower <= x <= upper of F(x) + radius * sum_i |(Dw x)_i|_2, F smooth with
 * grad F(x) = g + c_damp x, over a volume of nr x ne x na float64 voxels (row-major, a fastest).
 * (Dw x)_i is the triple of voxel i's weighted forward differences, Dw_ax = w_ax D_ax, with D_ax,
 * its edges, their owners and the azimuth ring exactly as sphrt_pd.h defines them; an axis has
 * edges iff w_ax > 0 and its length is > 1, and an edge that voxel i lacks contributes 0 to its
 * norm.  The conjugate of the term is the indicator of |q_i|_2 <= radius per voxel; the dual q is
 * three volumes, q + ax * n for ax = r, e, a (n = nr * ne * na), and slots without an edge are
 * never read or written.
 *
 * Launch shape, partition, sphrt_loss_partials and the order of the partial sums are those of
 * sphrt_pd.h: 256 threads, at most 1024 workgroups, grid-stride, element i owned by workgroup
 * (i / 256) mod grid; part_* receive one sum per workgroup.  Every fma stated below is one fma
 * and every other product a plain multiply, whatever -ffp-contract says; inf, NaN and denormals
 * are not special-cased.  `tau` and `sigma` point to one float64 each on the device.  Loads are
 * plain coalesced 8-byte loads, neighbours come from cache (no LDS tile).  Each entry fails on the
 * host, before any launch and without reading a pointer, on a null buffer, on buffers that
 * overlap, on an axis length < 1, on n >= 2^31, on a weight that is not finite and >= 0, on
 * (primal) a NaN bound or lower >= upper and on (dual) a radius that is not finite and >= 0.
 *
 * Feasibility of the dual.  The interval clamp of sphrt_pd_dual_f64 stores the bound's own bits;
 * a projection onto a ball cannot, but its excess is bounded.  Write u = 2^-53 and let v be the
 * triple before the projection, with exact squared norm N2 = sum v_ax^2.  Each square carries one
 * rounding and the two additions one each, all terms >= 0, so the computed n2 = N2 (1 + d1) with
 * |1 + d1| within (1 + u)^3 either way.  The correctly rounded square root gives nrm =
 * sqrt(n2) (1 + d2) with |d2| <= u, i.e. nrm >= sqrt(N2) (1 + u)^-1.5 (1 + u)^-1: a factor
 * (1 + u)^2.5 between nrm and |v|_2 at the most.  scale = radius / nrm carries one rounding and
 * each product v_ax * scale one more, so every stored |q_ax| <= |v_ax| (radius / |v|_2)
 * (1 + u)^4.5, and
 *
 *     sum_ax q_ax^2 <= radius^2 (1 + u)^9 < radius^2 (1 + 12 u)
 *
 * when the projection acts; when it does not (nrm <= radius) the same chain read backwards gives
 * |v|_2 <= radius (1 + u)^2.5, inside the same bound.  Denormal results (underflow in a square or
 * in a product) are outside this count, as they are outside every relative bound: there the
 * excess is absolute, below 2^-1022 per term.  |v_ax| > 1e154 overflows n2 to +inf: nrm = +inf,
 * scale = +0.0 for a finite radius and q_i = +-0 — a feasible store, not the projection; an inf
 * in v makes inf * 0 = NaN.  Neither is guarded.
 */
#ifndef SPHRT_ISO_H
#define SPHRT_ISO_H

#include "sphrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/*   gp = fma(c_damp, x[i], g[i])
 *   s  = (Dw^T q)[i]: from +0.0, over the edges present at i in the order r-, r+, e-, e+, a-, a+:
 *        s = fma( w_ax, q_ax[lower neighbour of i], s) for the edge arriving at i,
 *        s = fma(-w_ax, q_ax[i], s)                    for the edge leaving i
 *   u  = fma(-*tau, gp + s, x[i]);  x_new[i] = u < lower ? lower : (u > upper ? upper : u)
 *   part_mm: partial sums of (x_new[i] - x[i])^2
 * lower / upper: -inf / +inf for no bound.  x, g, x_new: n elements; q: 3 n.  With w_r = w_e =
 * w_a = 1 every fma above is exact in its product, and the result is bit for bit that of
 * sphrt_pd_primal_f64 with has_r = has_e = has_a = 1 (one kernel body, instantiated twice).    */
int sphrt_iso_primal_f64(const double *x, const double *g, const double *q, double *x_new,
                         int nr, int ne, int na, int wrap_a, double w_r, double w_e, double w_a,
                         double c_damp, const double *tau, double lower, double upper,
                         double *part_mm, void *stream);
/*   xb(j) = fma(2, x_new[j], -x_old[j]), formed at i and at its upper neighbours
 *   for ax = r, e, a with an edge leaving i, j its upper neighbour:
 *     e_ax = w_ax * (xb(j) - xb(i));  v_ax = fma(*sigma, e_ax, q_ax[i])
 *   n2  = v_r * v_r + v_e * v_e + v_a * v_a, the present axes only, added in the order r, e, a
 *         onto +0.0
 *   nrm = sqrt(n2), correctly rounded
 *   nrm > radius:  scale = radius / nrm;  q_ax[i] = v_ax * scale
 *   otherwise (a NaN nrm included):       q_ax[i] = v_ax        (in place: its own thread's slots)
 *   part_qq: partial sums of the voxels' terms, a voxel's term being the present axes' (q_ax[i]
 *   new - q_ax[i] old)^2 added in the order r, e, a onto +0.0                                  */
int sphrt_iso_dual_f64(const double *x_new, const double *x_old, double *q,
                       int nr, int ne, int na, int wrap_a, double w_r, double w_e, double w_a,
                       double radius, const double *sigma, double *part_qq, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPHRT_ISO_H */
