/*
 * sphrt_dp.h — C ABI of the diagonally preconditioned Chambolle-Pock iteration (libsphrt.so,
 * gfx950): what retrieval.chambolle_pock(precondition='diagonal') launches in place of the scalar
 * primal step of sphrt_pd.h and the scalar ray dual of sphrt_cp.h, and the one launch that forms
 * its steps.  Same conventions as sphrt.h (plain C types, caller-owned device buffers, `stream` a
 * hipStream_t passed as void*, 0 on success, otherwise a message in sphrt_last_error); a header of
 * its own so that the tables of the other three headers' entries, which other files are held to,
 * stay as they are.
 *
 * The steps are those of Pock and Chambolle (2011), Lemma 2 with alpha = 1, for K = [A; D]: A >= 0
 * entrywise with row sums row_i and column sums col_j, D the unweighted forward difference of
 * sphrt_pd.h (every edge row of |D| sums to 2, column j of |D| to deg_j, the number of edges
 * incident on voxel j).  With rho > 0 and c >= 0 (the damping term's curvature):
 *
 *   sigma_i = rho / row_i                      (+0.0 where row_i is not > 0)
 *   sigma_tv = rho / 2                         (the caller's: one float64 on the device, read by
 *                                               sphrt_pd_dual_f64 as its sigma)
 *   tau_j = 1 / fma(rho, col_j + deg_j, c)     (+0.0 where that denominator is not > 0)
 *
 * Launch shape, partition, sphrt_loss_partials and the order of the partial sums are those of the
 * loss entries of sphrt.h: 256 threads, at most 1024 workgroups, grid-stride, element i owned by
 * workgroup (i / 256) mod grid; part_* receive one sum per workgroup.  Every product that feeds a
 * sum is a plain multiply and the updates are the fmas written below, whatever -ffp-contract
 * says; division and sqrt are the correctly rounded IEEE ones; inf, NaN and denormals are not
 * special-cased beyond the guards written here (a NaN fails both compares of a clamp and stays
 * NaN).
 */
#ifndef SPHRT_DP_H
#define SPHRT_DP_H

#include "sphrt_cp.h"
#include "sphrt_pd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sphrt_pd_primal_f64 with a step per voxel: gp, s (the same order r-, r+, e-, e+, a-, a+) and
 * the clamp as there, and
 *   u = fma(-tau[i], gp + s, x[i]);  x_new[i] = u < lower ? lower : (u > upper ? upper : u)
 *   part_mm: partial sums of (x_new[i] - x[i])^2
 * x, g, x_new, tau: n = nr * ne * na elements; q: 3 n.  Fails on the host as sphrt_pd_primal_f64
 * does (a null buffer, an axis length < 1, n >= 2^31, a NaN bound or lower >= upper, buffers that
 * overlap, tau against an output among them).                                                  */
int sphrt_dp_primal_f64(const double *x, const double *g, const double *q, double *x_new,
                        int nr, int ne, int na, int wrap_a, int has_r, int has_e, int has_a,
                        double c_damp, const double *tau, double lower, double upper,
                        double *part_mm, void *stream);

/* sphrt_cp_ray_dual_f64 with a step per ray: thread j, i = order ? order[j] : j, reads
 * sg = sigma[i] (n elements, indexed as ray_scale is) where that entry reads *sigma; every other
 * operation, the four kinds, the rule s == 0 -> +0.0, p, p_adj, part_pp and part_fid are that
 * entry's, and so are its failures on the host.                                                 */
int sphrt_dp_ray_dual_f64(const double *z_new, const double *z_old, const void *y, int y_is_f64,
                          int64_t n, int kind, double delta_or_eps,
                          const double *ray_scale, const double *weight,
                          const double *sigma, const int32_t *order,
                          double *p, double *p_adj,
                          double *part_pp, double *part_fid, void *stream);

/* One launch over max(n_vox, n_ray) elements, n_vox = nr * ne * na:
 *   j < n_vox:  deg = the number of edges at voxel j, from its indices alone: per axis that has
 *               edges (has_ax != 0 and a length > 1) one for the edge arriving at j and one for
 *               the edge leaving it, as sphrt_pd.h counts them (with wrap_a and na = 2 both
 *               edges of the pair count at either voxel: 2 from that axis);
 *               d = fma(rho, col[j] + deg, c);  tau[j] = d > 0 ? 1 / d : +0.0
 *   j < n_ray:  r = row[order ? order[j] : j];  sigma[j] = r > 0 ? rho / r : +0.0
 * (a NaN fails the compare: +0.0).  `order` (null, or n_ray entries in 0 .. n_ray - 1) puts sigma
 * into the order a loop's forward writes when `row` is in another.  col, tau: n_vox elements;
 * row, sigma: n_ray.  Fails on the host, before any launch and without reading a pointer, on a
 * null buffer (order may be null), an axis length < 1, n_vox >= 2^31, n_ray < 1 or >= 2^31, a rho
 * that is not finite and > 0, a c that is not finite and >= 0, and on an output (tau, sigma) that
 * overlaps another buffer.                                                                      */
int sphrt_dp_steps_f64(const double *col, const double *row, int64_t n_ray,
                       int nr, int ne, int na, int wrap_a, int has_r, int has_e, int has_a,
                       double rho, double c, const int32_t *order,
                       double *tau, double *sigma, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPHRT_DP_H */
