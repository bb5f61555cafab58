/*
 * sphrt_cp.h — C ABI of the Chambolle-Pock solver's ray side (libsphrt.so, gfx950): the one
 * launch retrieval.chambolle_pock adds to the operator's own and to the two of sphrt_pd.h per
 * iteration.  Same conventions as sphrt.h (plain C types, caller-owned device buffers, `stream`
 * a hipStream_t passed as void*, 0 on success, otherwise a message in sphrt_last_error); a header
 * of its own so that the tables of sphrt.h's and sphrt_pd.h's entries, which other files are held
 * to, stay as they are.
 *
 * The problem: min over the box of sum_i phi_i((A x)_i) + (smooth and TV terms), the fidelity
 * dualised: a dual p_i per ray, updated by the proximal map of sigma phi_i^* at
 * a = p_i + sigma (2 z_new_i - z_old_i), z = A x.  With s = ray_scale[i] >= 0 (lam w_i / M) and
 * m = y[i]:
 *
 *   SPHRT_CP_SQUARE   phi(z) = s (z - m)^2                   prox: (a - sigma m) / (1 + sigma/(2s))
 *   SPHRT_CP_ABS      phi(z) = s |z - m|                     prox: clamp(a - sigma m, +-s)
 *   SPHRT_CP_HUBER    phi(z) = s huber_delta(z - m)          prox: clamp((a - sigma m) / (1 + sigma/s),
 *                                                                        +-s delta)
 *   SPHRT_CP_POISSON  phi(z) = s (z - m log(z + eps))        prox: the smaller root of
 *                     p^2 - (a' + s) p + (a' s - sigma s m) = 0, a' = a + sigma eps, never above s
 *
 * Launch shape, partition, sphrt_loss_partials and the order of the partial sums are those of the
 * loss entries of sphrt.h: 256 threads, at most 1024 workgroups, grid-stride, thread j of the
 * launch owned by workgroup (j / 256) mod grid; part_* receive one sum per workgroup.  Every
 * product that feeds a sum is a plain multiply and the updates are the fmas written below,
 * whatever -ffp-contract says; division and sqrt are the correctly rounded IEEE ones; inf, NaN
 * and denormals are not special-cased (a NaN fails both compares of a clamp and stays NaN).
 */
#ifndef SPHRT_CP_H
#define SPHRT_CP_H

#include "sphrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPHRT_CP_SQUARE 0
#define SPHRT_CP_ABS 1      /* = SPHRT_RESID_ABS */
#define SPHRT_CP_HUBER 2    /* = SPHRT_RESID_HUBER */
#define SPHRT_CP_POISSON 3

/* Thread j, with i = order ? order[j] : j (order a permutation of 0 .. n - 1: each slot has one
 * owner), zn = z_new[i], zo = z_old[i], m = y[i] (float32 promoted exactly when !y_is_f64),
 * s = ray_scale[i], w = weight[i], po = p[i], sg = *sigma:
 *
 *   zb = fma(2, zn, -zo);  a = fma(sg, zb, po);  t = fma(-sg, m, a)
 *   SQUARE   pn = t / (1 + sg / (2 s))
 *   ABS      pn = t < -s ? -s : (t > s ? s : t)
 *   HUBER    u = t / (1 + sg / s);  b = s * delta;  pn = u < -b ? -b : (u > b ? b : u)
 *   POISSON  a' = fma(sg, eps, a);  d = a' - s;  e = a' + s
 *            D = fma((4 sg) * s, m, d * d);  v = 0.5 * (e - sqrt(D));  pn = v > s ? s : v
 *   every kind: s == 0 gives pn = +0.0, whatever the other operands hold
 *   p[i] = pn; with order, p_adj[j] = pn (the stored adjoint's input in trace order, as
 *   sphrt_sq_residual_f64 uses `order`)
 *   part_pp:  partial sums of (pn - po)^2
 *   part_fid: partial sums of w * rho(zn, m), rho op for op that of the residual entries: with
 *             r = zn - m: r * r (SQUARE), |r| (ABS), the Huber h of sphrt_robust_residual_f64, and
 *             zn - m * log(zn + eps) (POISSON)
 *
 * delta_or_eps: the Huber delta or the Poisson eps (finite and > 0), ignored by the other kinds.
 * Fails on the host, before any launch and without reading a pointer, on n <= 0, a null buffer
 * (order and p_adj may be null only together), an unknown kind, a delta / eps that is not finite
 * and > 0, and on an output (p, p_adj, part_pp, part_fid) that overlaps another buffer.          */
int sphrt_cp_ray_dual_f64(const double *z_new, const double *z_old, const void *y, int y_is_f64,
                          int64_t n, int kind, double delta_or_eps,
                          const double *ray_scale, const double *weight,
                          const double *sigma, const int32_t *order,
                          double *p, double *p_adj,
                          double *part_pp, double *part_fid, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPHRT_CP_H */
