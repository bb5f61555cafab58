/*
 * sphrt.h — C ABI of the MI355X-native spherical-grid raytracer (libsphrt.so, gfx950).
 *
 * This is the drop-in boundary for the hot path of Evidlo/sph_raytracer: ray <-> spherical-voxel
 * intersection (sphere / cone / half-plane crossings), per-ray merge + forward fill + segment
 * lengths, and the line-integral forward / adjoint.  The reference has no native boundary; its
 * interface is the Python `Operator` (raytracer.py:647-755).  Each entry point below names the
 * reference code it replaces.  The Python package `sph_raytracer_amd` binds these with ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - Plain C types only.  Every large buffer is allocated by the caller (PyTorch-ROCm tensors) and
 *    passed as a raw device pointer; the library never frees caller memory.  A plan owns only its
 *    small boundary tables.
 *  - `stream` is a hipStream_t passed as void*.  All work is stream-ordered; the only host sync in
 *    the whole trace is the caller's read of the total segment count between count and fill.
 *    Every call launches on its stream's device, whatever device is current in the calling
 *    thread (a null stream means the current device's); calls with a plan fail when the stream
 *    is not on the plan's device.
 *  - Return value: 0 on success, non-zero on error; sphrt_last_error() gives a message
 *    (thread-local).  Functions never abort the process.
 *  - Geometry is float64 (reference FTYPE = float64, raytracer.py:14).  Densities / images may be
 *    float32 or float64 (float64 densities are accumulated in float64; float32 ones: see
 *    sphrt_forward_f32).
 */
#ifndef SPHRT_H
#define SPHRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPHRT_MAX_DIMS 6

/* Boundary description of a SphericalGrid (geometry.py:107-183).  All pointers are HOST memory;
 * the trigonometric tables are computed by the caller with the same host library the reference
 * uses (torch CPU: raytracer.py:373-375, 505-506), so every table entry is bit-identical. */
typedef struct sphrt_grid_desc {
    int32_t nr, ne, na;       /* voxels per axis: grid.shape.r/e/a                              */
    const double *r_b;        /* nr+1 sphere radii, ascending            (geometry.py:158-161)  */
    const double *e_b;        /* ne+1 cone angles from +Z                (geometry.py:165)      */
    const double *a_b;        /* na+1 half-plane azimuths                (geometry.py:166)      */
    const double *cos_e;      /* torch.cos(e_b)                          (raytracer.py:452)     */
    const double *cos2_e;     /* torch.cos(e_b)**2                       (raytracer.py:373-375) */
    const double *cos_a;      /* torch.cos(a_b)                          (raytracer.py:505)     */
    const double *sin_a;      /* torch.sin(a_b)                          (raytracer.py:506)     */
    int32_t a_wrap;           /* -a_b[0] == a_b[-1] == pi                (raytracer.py:528)     */
    double close_tol;         /* finfo(ftype).resolution ** (1/3)        (raytracer.py:233-246) */
    double plane_par_tol;     /* finfo(ftype).resolution                 (raytracer.py:521)     */
} sphrt_grid_desc;

typedef struct sphrt_plan sphrt_plan;

/* Ray batch: `ndim`-dimensional broadcast shape; xs (...,3) f64 ray starts and rays (...,3) f64
 * directions addressed with per-dim element strides (0 = broadcast dim), last dim contiguous.
 * `start` holds the start voxel of every *unique* start as int32 (r, e, a, pad), addressed as
 * start[4 * (xs_offset / 3)] — i.e. laid out like an un-broadcast, contiguous xs.  It replaces
 * find_starts (raytracer.py:605-644), which the caller evaluates on the host once per unique
 * start. */
typedef struct sphrt_rays {
    int32_t ndim;
    int64_t shape[SPHRT_MAX_DIMS];
    int64_t xs_stride[SPHRT_MAX_DIMS];
    int64_t rays_stride[SPHRT_MAX_DIMS];
    const double *xs;
    const double *rays;
    const int32_t *start;
} sphrt_rays;

/* ---- plan --------------------------------------------------------------------------------- */
/* Replaces the per-call conversion of grid.r_b/e_b/a_b inside r_torch/e_torch/a_torch
 * (raytracer.py:271-277, 353-361, 493-501).  `device` is the HIP device ordinal. */
int sphrt_plan_create(const sphrt_grid_desc *grid, int device, sphrt_plan **out);
/* The same plan over caller-owned device tables (no hipMalloc, no hipFree: the device-wide sync
 * hipFree implies is avoided): sphrt_plan_pack_tables writes sphrt_plan_table_bytes(grid) bytes
 * into host memory, the caller copies them to an 8-byte-aligned device buffer that outlives the
 * plan (stream-ordered before the plan's first use) and passes it here. */
size_t sphrt_plan_table_bytes(const sphrt_grid_desc *grid);
int sphrt_plan_pack_tables(const sphrt_grid_desc *grid, void *host_tables);
int sphrt_plan_create_external(const sphrt_grid_desc *grid, int device, const void *dev_tables,
                               sphrt_plan **out);
int sphrt_plan_destroy(sphrt_plan *plan);
/* Candidates per ray in the reference's concatenation (raytracer.py:92, 117-122):
 * K = 2(nr+1) + 2(ne+1) + (na+1) + 1. */
int64_t sphrt_plan_candidates(const sphrt_plan *plan);
const char *sphrt_last_error(void);
const char *sphrt_version(void);

/* ---- per-family crossing solves (API-parity with r_torch / e_torch / a_torch) -------------- */
/* family 0 = spheres  (r_torch, raytracer.py:248-325): t, region  (n, 2*(nr+1))
 * family 1 = cones    (e_torch, raytracer.py:328-468): t, region  (n, 2*(ne+1))
 * family 2 = planes   (a_torch, raytracer.py:471-552): t, region  (n, na+1)
 * `neg` receives negative_crossing (int8, same shape).  Rays are normalised on private copies
 * (the reference normalises the caller's tensor in place, raytracer.py:281/365). */
int sphrt_solve(const sphrt_plan *plan, const sphrt_rays *rays, int family,
                double *t, int32_t *region, int8_t *neg, void *stream);
/* The same solves in float32 (r_torch / e_torch / a_torch with ftype=torch.float32): starts and
 * directions rounded to float, every operation in float.  The plan must hold the float32 tables
 * (boundaries, cos/sin evaluated by torch in float32, stored exactly as doubles) and the float32
 * thresholds (close_tol = 1e-6 ** (1/3), plane_par_tol = 1e-6: raytracer.py:233-246, 521). */
int sphrt_solve_f32(const sphrt_plan *plan, const sphrt_rays *rays, int family,
                    float *t, int32_t *region, int8_t *neg, void *stream);

/* ---- trace to compact CSR (replaces trace_indices, raytracer.py:48-230) -------------------- */
/* Every trace call takes a caller-allocated device workspace of
 * sphrt_trace_workspace_bytes(plan, n) bytes: it holds the list of rays whose crossings tie
 * exactly in a way that makes the result depend on the reference's (unstable, libstdc++
 * introsort) tie order, and the scratch of the exact kernel that replays that order. */
size_t sphrt_trace_workspace_bytes(const sphrt_plan *plan, int64_t n);
/* Pass 1: number of non-zero-length, in-grid segments of every ray (int32, n = prod(shape)). */
int sphrt_trace_count(const sphrt_plan *plan, const sphrt_rays *rays, int32_t *counts,
                      void *workspace, size_t workspace_size, void *stream);
/* Exclusive scan counts -> row_ptr (n+1, int64).  `workspace` must hold
 * sphrt_scan_workspace_bytes(n) bytes.  row_ptr[n] is the total segment count. */
size_t sphrt_scan_workspace_bytes(int64_t n);
int sphrt_scan_counts(const int32_t *counts, int64_t n, int64_t *row_ptr, void *workspace,
                      void *stream);
/* Pass 2: per-segment linear voxel index ((r*ne + e)*na + a) and length, in ray order and, per
 * ray, in order of increasing distance.  Equivalent to the reference's (regs, lens) with
 * zero-length and invalid entries dropped (raytracer.py:131-173). */
int sphrt_trace_fill(const sphrt_plan *plan, const sphrt_rays *rays, const int64_t *row_ptr,
                     int32_t *vox, double *len, void *workspace, size_t workspace_size,
                     void *stream);

/* Reference-mode trace: the options the fast trace does not take (Operator(..., ftype=float32)
 * and / or invalid=True, raytracer.py:48-173).  Every ray runs the reference algorithm verbatim
 * on the device: all K candidates, its (unstable) introsort order, the forward fill and the
 * length differences.  flags: SPHRT_TRACE_F32 — solves and differences in float32 (a float32
 * plan, as for sphrt_solve_f32; lengths are float32 values stored as doubles);
 * SPHRT_TRACE_INVALID — no masking (raytracer.py:155 `if not invalid`): every non-zero length is
 * kept, inf and NaN included, with its voxel wrapped the way the reference's forward indexes it
 * (region -1 reads the last shell / cone / wedge); SPHRT_TRACE_FRESH_RAYS — the caller's rays are
 * not of the trace's dtype, so tr.asarray(rays, ftype) hands each solver a fresh copy
 * (raytracer.py:276,360,500): r_torch and e_torch normalise theirs once, a_torch uses them
 * unnormalised (without the flag the in-place normalisations of raytracer.py:281,365 chain: e_torch
 * and a_torch see the twice-normalised rays).  row_ptr == NULL: count pass (`counts`, int32 per
 * ray); else fill pass into (vox, len) at row_ptr.  Workspace: sphrt_trace_workspace_bytes. */
#define SPHRT_TRACE_F32 1
#define SPHRT_TRACE_INVALID 2
#define SPHRT_TRACE_FRESH_RAYS 4
int sphrt_trace_reference(const sphrt_plan *plan, const sphrt_rays *rays, int flags,
                          int32_t *counts, const int64_t *row_ptr, int32_t *vox, double *len,
                          void *workspace, size_t workspace_size, void *stream);
/* The reference-mode trace in one pass, as sphrt_trace_emit: every ray's segments into its slot
 * [bound_ptr[i], bound_ptr[i+1]) of (svox, slen) and its exact count into counts; rays whose
 * count exceeds their slot write only the count and are counted in *n_over (device int64).  A
 * slot of K (sphrt_plan_candidates) segments always suffices: the walk keeps at most one segment
 * per list entry.  Compact with sphrt_trace_compact after scanning the counts. */
int sphrt_trace_reference_emit(const sphrt_plan *plan, const sphrt_rays *rays, int flags,
                               const int64_t *bound_ptr, int32_t *counts, int32_t *svox,
                               double *slen, int64_t *n_over, void *workspace,
                               size_t workspace_size, void *stream);

/* One-pass trace (the same CSR as count + fill, tracing every ray once instead of twice):
 *  1. sphrt_trace_bound: screens the rays and writes an upper bound of every ray's segment count
 *     from its geometry alone (int32 `bounds`, 0 for rays that miss the grid); the caller scans
 *     them (sphrt_scan_counts) into bound_ptr (n+1) and allocates a staging CSR of
 *     bound_ptr[n] entries (svox int32, slen float64).
 *  2. sphrt_trace_emit (same workspace: it traces the hit list step 1 left there): every ray's
 *     exact segment count into `counts`, and its segments into staging slot
 *     [bound_ptr[ray], bound_ptr[ray+1]) when they fit.  *n_over (device int64) = rays that did
 *     not fit; if it is non-zero the staging is incomplete and the caller runs sphrt_trace_fill
 *     instead of step 3 (the counts are exact either way).
 *  3. after sphrt_scan_counts(counts) -> row_ptr: sphrt_trace_compact moves the rows into the
 *     tight CSR (vox, len: row_ptr[n] entries).  Either pair (svox, vox) or (slen, len) may be
 *     NULL to move the other one alone: moving them in two calls, freeing each staging array
 *     after its call, caps the peak footprint at staging + 12 B per segment. */
int sphrt_trace_bound(const sphrt_plan *plan, const sphrt_rays *rays, int32_t *bounds,
                      void *workspace, size_t workspace_size, void *stream);
int sphrt_trace_emit(const sphrt_plan *plan, const sphrt_rays *rays, const int64_t *bound_ptr,
                     int32_t *counts, int32_t *svox, double *slen, int64_t *n_over,
                     void *workspace, size_t workspace_size, void *stream);
int sphrt_trace_compact(int64_t n, const int64_t *bound_ptr, const int32_t *svox,
                        const double *slen, const int64_t *row_ptr, int32_t *vox, double *len,
                        void *stream);

/* TEST HOOK (tests/test_gpu_exact_sort.py): the sorts of the exact path — the device emulation of
 * the reference's unstable torch.sort — on lists handed in from the host, one workgroup per list.
 * t: n_lists x K distances in the trace's concatenation order; reg: the region every entry writes
 * (the device forms pay = index << 16 | (reg + 2) as the trace does; reg in [-2, 65533]); start:
 * three int32 per list, the start voxel; nbr / nbe: boundary counts, entries below 2 nbr are
 * sphere crossings, below 2 nbr + 2 nbe cone crossings, then half-planes, entry K - 1 the start
 * entry.  method:
 *   SPHRT_SORT_SERIAL_AOS  the serial emulation on one lane over a global-memory list (grids whose
 *                          list does not fit LDS); workspace: sphrt_exact_sort_workspace_bytes
 *   SPHRT_SORT_SERIAL_SOA  the same on one lane over the LDS list (the wave kernel's NaN fallback)
 *   SPHRT_SORT_WAVE1 / 4   the wave-parallel emulation with one wave / four waves per list;
 *                          `invalid` selects the invalid=True instantiation (ties of infinite
 *                          distances matter)
 *   SPHRT_SORT_NETWORK     the reference mode's register sort alone; a list it refuses writes only
 *                          its flag, nothing falls back
 * Writes the sorted distances (t_out) and payloads (pay_out), n_lists x K each, and per list
 * SPHRT_SORT_INFO_FIELDS int64 `info`: depth-limit ranges rank-sorted, heap-sorted (wave methods),
 * the network's accepted flag, 1 when a wave method met a NaN (it then sorts nothing).  Lists must
 * hold no NaN, except for SPHRT_SORT_NETWORK: the serial emulation's unguarded scans are
 * undefined over NaN, as std::sort's are.  A K outside [1, sphrt_exact_sort_max_k(method)] is an
 * error (the network: [2, 512]; -1 for an unknown method). */
#define SPHRT_SORT_SERIAL_AOS 0
#define SPHRT_SORT_SERIAL_SOA 1
#define SPHRT_SORT_WAVE1 2
#define SPHRT_SORT_WAVE4 3
#define SPHRT_SORT_NETWORK 4
#define SPHRT_SORT_INFO_FIELDS 4
int64_t sphrt_exact_sort_max_k(int method);
size_t sphrt_exact_sort_workspace_bytes(int method, int64_t n_lists, int64_t K);
int sphrt_exact_sort_lists(const double *t, const int32_t *reg, const int32_t *start,
                           int64_t n_lists, int64_t K, int32_t nbr, int32_t nbe, int method,
                           int invalid, double *t_out, uint32_t *pay_out, int64_t *info,
                           void *workspace, size_t workspace_size, void *stream);

/* ---- on-device cone-beam ray directions (replaces ConeRectGeom.rays, geometry.py:493-508, and
 * ConeCircGeom.rays, geometry.py:570-582) ----------------------------------------------------- */
/* rays[v][a][b][0..2] for n_views views of h x w pixels, bit-identical to the torch expressions.
 * frame: per view {lookdir, lookdir x updir, updir} (9 doubles).  circ == 0 (rect): row[v][a] =
 * linspace(-ulim, ulim, h), col[v][b] = linspace(-vlim, vlim, w).  circ == 1: row[v][a] = r,
 * col[v] = {cos(theta) (w values), sin(theta) (w values)}, r*cos and r*sin in double; circ == 2:
 * the same with r*cos and r*sin rounded to float (the host tensors are float32). */
int sphrt_rays_cone(int64_t n_views, int64_t h, int64_t w, int circ, const double *frame,
                    const double *row, const double *col, double *rays, void *stream);
/* The same rays in a per-view trace order (the ConeCirc wedge order of the Operator's trace):
 * rays[v][k] is pixel order[k] of view v (order: a permutation of the h*w pixels, device
 * memory) and ray_id[v*h*w + k] = v*h*w + order[k] (int32; n_views*h*w < 2^31). */
int sphrt_rays_cone_ordered(int64_t n_views, int64_t h, int64_t w, int circ, const double *frame,
                            const double *row, const double *col, const int64_t *order,
                            double *rays, int32_t *ray_id, void *stream);
/* The same rays in tiles across views: rays is laid out (h, w / tw, n_views / tv, tv, tw, 3) —
 * each tile holds tw neighbouring pixels of one detector row seen from tv consecutive views —
 * and ray_id[i] = the geometry ray (v * h * w + pixel) of row i (int32; n_views * h * w < 2^31).
 * tv must divide n_views and tw must divide w.  The Operator traces orbits in this order
 * (raytracer._view_tiles); ray starts broadcast over it with per-dim strides (sphrt_rays). */
int sphrt_rays_cone_tiled(int64_t n_views, int64_t h, int64_t w, int circ, const double *frame,
                          const double *row, const double *col, int64_t tv, int64_t tw,
                          double *rays, int32_t *ray_id, void *stream);

/* ---- row index of the trace, built once (the apply kernels' work partition) ---------------- */
/* A traced operator: the CSR above plus
 *   vox     — bit 31 (SPHRT_ROW_HEAD) set on the first segment of every non-empty ray,
 *   row_ray — ray id of every non-empty row, in order,
 *   empty_ray — the rays without segments, ascending (allocate n_rays + 1 entries),
 *   blocks  — n_blocks x 6 int64 {empty_lo, empty_hi, seg_lo, seg_hi, row_lo, n_tab}: block b
 *             owns the whole rows starting in segments [b*1792, (b+1)*1792) (b*1984 with dense
 *             output ranges: sphrt_csr_index_dense) and zeroes the empty
 *             rays empty_ray[empty_lo .. empty_hi),
 *   tab     — (optional) per block b, its n_tab distinct 4-voxel granules (voxel >> 2) ascending
 *             at tab[b*tab_stride ..) (n_blocks * tab_stride entries),
 *   loc     — (optional) per segment, 16 * (rank of its granule in the block's table + 1) +
 *             4 * (voxel & 3): the voxel's byte offset in the forward's float LDS image, whose
 *             granule 0 is zero; the row-head flag in bit 15 (SPHRT_LOC_HEAD).
 * sphrt_csr_index() fills vox heads, row_ray, empty_ray and blocks from row_ptr (n_tab = -1);
 * n_blocks = sphrt_csr_blocks(n_segments).  sphrt_csr_local_count/_fill then build tab and loc
 * (uint16, n_segments entries) for every block of at most 4096 segments and 2046 granules; with
 * loc/tab/n_cols/tab_stride set, a static forward on a 16-byte-aligned density stages each
 * block's granules in LDS (4 * (tab_stride + 1) elements, up to 64 KB) instead of gathering per
 * segment; sphrt_forward_plan makes that choice and reports it.
 * Per-segment arrays (vox, len, len32, loc) are read in aligned 8- or 16-entry chunks: allocate
 * them to round_up(n_segments, 16) entries (the entries past n_segments are never used).  `len32` is
 * the float32 copy of `len` used by the float32 forward: sphrt_csr_local_count / _build write it
 * (len32[i] = (float)len[i], every segment) when both len and len32 are set, else the caller makes
 * it (sphrt_f64_to_f32). */
#define SPHRT_ROW_HEAD 0x80000000u
#define SPHRT_BLOCK_FIELDS 6   /* int64 per entry of blocks */
#define SPHRT_LOC_HEAD 0x8000u
/* Forward workgroups resident at once on an MI355X (256 CUs x 6): grids up to this size run as one
 * wave.  The block order (sphrt_csr.order), the staged build's row search and the Python layer's
 * brick / alternation rules all switch here. */
#define SPHRT_SINGLE_WAVE_BLOCKS 1536
typedef struct sphrt_csr {
    int64_t n_rays;
    int64_t n_segments;
    const int64_t *row_ptr;
    const int32_t *vox;
    const double *len;
    const float *len32;
    const int32_t *row_ray;
    const int64_t *blocks;
    int64_t n_blocks;
    const uint16_t *loc;   /* NULL: per-segment gathers through vox */
    const void *tab;       /* int32 entries, or uint16 when tab_bytes == 2 */
    int64_t n_cols;        /* column ids (vox & ~head) are < n_cols: voxels, or rays if transposed */
    int64_t n_fallback;    /* blocks without a granule table (n_tab = -1), from sphrt_csr_local */
    const int32_t *empty_ray;  /* the rays without segments, ascending (n_rays - rows entries) */
    int64_t tab_stride;    /* granule-table entries per block (>= the largest n_tab) */
    int64_t tab_bytes;     /* 2: uint16 table entries (n_cols <= 2^18), else int32 */
    /* Brick staging for the granule-table forward (all zero: off).  The columns are the voxels of
     * an (Nr, Ne, Na) = stage_shape grid; the granule tables and loc address a copy of the
     * density re-laid in bricks of stage_brick = (br, be, ba) voxels (each dim padded up to a
     * multiple of its brick), so one 128-byte line holds a compact 3-D neighbourhood instead of a
     * run along a.  Every table-mode forward first packs the density into `stage` (stage_bytes,
     * >= n_chan * stage_cols * sizeof(T), else the call fails).  The stage is scratch of one call:
     * two calls in flight at once (e.g. on two streams) need two stage buffers; the Python layer
     * passes a fresh stream-ordered allocation with every call.  vox stays in natural order. */
    int32_t stage_shape[3];
    int32_t stage_brick[3];
    int64_t stage_cols;    /* prod over dims of ceil(shape / brick) * brick */
    void *stage;
    int64_t stage_bytes;
    /* (optional, sphrt_csr_runs) per block SPHRT_RUN_FIELDS int32: its rows' rays and its share
     * of the empty rays as ranges; NULL: the forward reads row_ray / empty_ray instead. */
    const int32_t *runs;
    /* Block order of the forward (a performance hint: results are identical).  0: the default
     * order; bit 0 set: reversed; bit 1 set: one contiguous range of blocks per XCD, for CSRs
     * whose rays read disjoint column ranges (the time-paired CSR of a dynamic grid: C4 forward
     * f32 20.3 -> 18.9 us).  The Python layer flips bit 0 after every launch of a CSR of more than one
     * resident wave of blocks, so a CSR (or a forward / adjoint pair) that outgrows the
     * memory-side cache starts each launch on the lines the previous launch left cached instead
     * of the ones it evicted first (C3 forward f32 233 -> 213 us; C5 retrieval 0.138 -> 0.133
     * ms/iteration).  Bit 2 set (not a hint: a layout): dense output ranges — the rows are in
     * output order (row_ray increasing) and each block record's fields 0 / 1 hold the output range
     * [lo, hi) that block writes, its rows and the empty rows up to the next block's first row;
     * the block zeroes the range itself and empty_ray is not read.  One channel, no
     * ray_chan_div, runs NULL. */
    int64_t order;
    /* 1: `stage` already holds this call's density in the brick layout (pad columns zero), e.g.
     * written by sphrt_adam_neg_f64 after an earlier forward packed the same buffer; the forward
     * skips its pack.  0: the forward packs (the default). */
    int64_t stage_packed;
} sphrt_csr;

int64_t sphrt_csr_blocks(int64_t n_segments);
size_t sphrt_csr_index_workspace_bytes(int64_t n_rays);
/* ray_ids: NULL (row r is ray r), or the ray each row reports in row_ray / empty_ray — the
 * output index of a trace made in another ray order than the geometry's (the Operator traces
 * ConeCirc views in wedges of raytracer._WEDGE (3) azimuth columns, raytracer._trace_order). */
int sphrt_csr_index(const int64_t *row_ptr, int64_t n_rays, int32_t *vox, int32_t *row_ray,
                    int32_t *empty_ray, int64_t *blocks, int64_t n_blocks, const int32_t *ray_ids,
                    void *workspace, void *stream);
/* The same index for a CSR that will take dense output ranges (order bit 2: rows in output order,
 * one output per row or empty row — the time-paired transposed adjoint): block b owns the rows
 * starting in segments [b*1984, (b+1)*1984), n_blocks = sphrt_csr_blocks_dense(n_segments).  The
 * forward reads a CSR with order bit 2 set by these blocks, so its index must come from here.
 * Its blocks zero their output ranges with 16-byte stores placed by element index: the
 * forward's `out` must be 16-byte aligned, and sphrt_forward_f32/_f64 refuse any other pointer
 * for such a CSR before launching anything. */
int64_t sphrt_csr_blocks_dense(int64_t n_segments);
int sphrt_csr_index_dense(const int64_t *row_ptr, int64_t n_rays, int32_t *vox, int32_t *row_ray,
                          int32_t *empty_ray, int64_t *blocks, int64_t n_blocks,
                          const int32_t *ray_ids, void *workspace, void *stream);
/* Granule tables in two passes.  _count sets n_tab in blocks (-1: no table) and writes two
 * device int64 to stats: {blocks without a table, largest n_tab}; the caller copies the first to
 * csr->n_fallback, picks tab_stride >= the second (csr->tab_stride; tab holds n_blocks *
 * tab_stride entries) and runs _fill.  Brick staging (stage_* fields) is decided before _count:
 * both passes and every later forward on the tables use the same stage_* values. */
int sphrt_csr_local_count(const sphrt_csr *csr, int64_t *blocks, int64_t *stats, void *stream);
int sphrt_csr_local_fill(const sphrt_csr *csr, const int64_t *blocks, uint16_t *loc, void *tab,
                         int64_t tab_stride, void *stream);
/* The same tables in one pass: _build decides n_tab (and the fallback blocks) and writes loc and
 * each kept block's table at the fixed wide stride SPHRT_TAB_WIDE (tab_wide: n_blocks *
 * SPHRT_TAB_WIDE entries of tab_bytes each), with stats as in _count; the caller picks tab_stride
 * from stats and _pack copies the tables to that stride.  Same output as _count + _fill. */
#define SPHRT_TAB_WIDE 2048
int sphrt_csr_local_build(const sphrt_csr *csr, int64_t *blocks, uint16_t *loc, void *tab_wide,
                          int64_t *stats, void *stream);
int sphrt_csr_local_pack(const sphrt_csr *csr, const int64_t *blocks, const void *tab_wide,
                         void *tab, int64_t tab_stride, void *stream);
/* The one-pass trace without its compaction pass (one-pass table build).  After sphrt_trace_emit the segments sit in staging slots (svox / slen at
 * slot[row], the scanned bounds); sphrt_csr_index_staged indexes the CSR from row_ptr alone (no
 * head bits: vox is not written yet) and lists the trace row of every non-empty row (nz_row, one
 * int32 per non-empty row: allocate n_rays); sphrt_csr_local_build_staged then moves every block's
 * segments from the staging into csr->vox (with the row-head bits), csr->len and csr->len32 and
 * builds the tables from them — the same CSR, loc and tables as sphrt_trace_compact +
 * sphrt_csr_index + sphrt_csr_local_build (csr->vox/len/len32 are written through the const
 * pointers).  The staging may be freed after it — except with csr->len NULL: the float64
 * lengths then stay in slen (the float32 forward reads len32 only) until
 * sphrt_trace_compact(svox = vox = NULL) moves them into the CSR on the first use that needs
 * them; svox may be freed right away. */
int sphrt_csr_index_staged(const int64_t *row_ptr, int64_t n_rays, int32_t *row_ray,
                           int32_t *empty_ray, int64_t *blocks, int64_t n_blocks,
                           const int32_t *ray_ids, int32_t *nz_row, void *workspace, void *stream);
int sphrt_csr_local_build_staged(const sphrt_csr *csr, int64_t *blocks, uint16_t *loc,
                                 void *tab_wide, int64_t *stats, const int64_t *slot,
                                 const int32_t *nz_row, const int32_t *svox, const double *slen,
                                 void *stream);
/* Row runs (optional).  Block b's rows map to rays in runs of consecutive rays, and its share of
 * the empty rays (empty_ray[empty_lo .. empty_hi)) to ranges of consecutive rays; when both fit
 * in SPHRT_MAX_RUNS entries for every block, the table-mode forward takes them from one 128-byte
 * record per block instead of loading row_ray / empty_ray entries (no dependent row loads, and
 * the empty rays are zeroed by contiguous stores).  runs: n_blocks x SPHRT_RUN_FIELDS int32
 *   [0] row runs, [1] empty ranges (-1: more than SPHRT_MAX_RUNS),
 *   [2 + 2i], [3 + 2i]  run i: first row (relative to the block's row_lo), its ray,
 *   [16 + 2i], [17 + 2i] empty range i: first ray, ray count.
 * Writes one device int64 to stats: the number of blocks with more than SPHRT_MAX_RUNS runs or
 * ranges (the caller sets csr->runs only when it is 0).  Needs row_ray, empty_ray and blocks. */
#define SPHRT_RUN_FIELDS 32
#define SPHRT_MAX_RUNS 7
int sphrt_csr_runs(const sphrt_csr *csr, int32_t *runs, int64_t *stats, void *stream);

/* Time-paired columns for a dynamic operator whose view i sees time slice i (ray r reads slice
 * r / div): vox_out[s] = (r / div) * vol + voxel, head bit kept, for every segment of ray r.  A
 * CSR with these columns (and its own blocks / tables, n_cols = T * vol) is a static CSR over the
 * flattened (T, vol) density: granule-table forward, transposed deterministic adjoint.
 * Requires T * vol < 2^31. */
int sphrt_csr_time_columns(const sphrt_csr *csr, int64_t div, int64_t vol, int32_t *vox_out,
                           void *stream);

/* ---- forward line integral on the CSR (replaces Operator.__call__, raytracer.py:692-713) -- */
/* out[c*out_chan_stride + i] = sum_s density[c*chan_stride + vox[s]] * len[s] over ray i's row.
 * If ray_chan_div > 0, ray i only sees channel c = i / ray_chan_div (dynamic grid paired with a
 * ViewGeomCollection, raytracer.py:705-706) and n_chan must be 1 in the call (the channel is
 * derived); otherwise every ray is integrated for all n_chan channels (static multichannel).
 * float64: products and sums in float64.  float32 (streams `len32`): products and each thread's
 * run of up to 8 consecutive segments of a row in float32 (the reference's own f32 product
 * rounding, raytracer.py:710), the runs of a row stitched across threads in float32 as well
 * (the reference sums in float32 too); measured within 2.5e-7 relative of float64
 * accumulation (C2-C5). */
int sphrt_forward_f32(const sphrt_csr *csr, const float *density, int64_t n_chan,
                      int64_t chan_stride, int64_t ray_chan_div, float *out,
                      int64_t out_chan_stride, void *stream);
int sphrt_forward_f64(const sphrt_csr *csr, const double *density, int64_t n_chan,
                      int64_t chan_stride, int64_t ray_chan_div, double *out,
                      int64_t out_chan_stride, void *stream);

/* Which forward_kernel instantiation sphrt_forward_f32/_f64 launch for a call, and how.  The
 * library decides this in one place and the forwards dispatch from the same record; callers read
 * it for reports only (the Python layer formats it into the kernel's name).  Flags are 0 / 1. */
typedef struct sphrt_fwd_plan {
    int32_t mode;             /* 0: granule tables staged in LDS, 1: per-segment gathers through
                                 vox, 2: time slices (ray_chan_div > 0)                          */
    int32_t tab_bytes;        /* width of the table entries read: 2 or 4 (4 when mode != 0)      */
    int32_t edma;             /* granule DMA issued before the block record (whole-granule cols) */
    int32_t runs;             /* rows' rays from the run records (sphrt_csr.runs)                */
    int32_t half;             /* float64 half tables: the LDS image holds half a table at a time */
    int32_t dense;            /* dense output ranges (sphrt_csr.order bit 2)                     */
    int32_t early_rounds;     /* 256-entry table chunks fetched early (the kernel's GE argument) */
    int32_t segs_per_thread;  /* segments per thread per pass (workgroups of 2048 / this)        */
    int32_t fallback;         /* a second, gather launch follows for the blocks without a table  */
    int32_t lds_bytes;        /* dynamic LDS per workgroup of the main launch                    */
    int32_t chunk;            /* block order: consecutive blocks dealt per XCD (0: dispatch
                                 order, INT32_MAX: one range per XCD; ~chunk: reversed)          */
    int32_t elem_bytes;       /* 4: float32 density, lengths and output, 8: float64              */
} sphrt_fwd_plan;
/* The plan of sphrt_forward_f32 (elem_bytes 4) / _f64 (8) called with these arguments.  Host code
 * only: no device is touched and no pointer is dereferenced except csr; `density` counts by its
 * address (granule alignment), and a brick-staged CSR's by its `stage` pointer (NULL: aligned).
 * Fails as the forward would on arguments it refuses before looking at `out` or the stage. */
int sphrt_forward_plan(const sphrt_csr *csr, int elem_bytes, const void *density, int64_t n_chan,
                       int64_t chan_stride, int64_t ray_chan_div, sphrt_fwd_plan *out);

/* Kernel timing for measurement (bench.py's roofline; no reference counterpart): the next
 * sphrt_forward_f32/f64 call on this host thread launches its main forward kernel with these two
 * HIP events (hipEvent_t, created with timing) bound to the dispatch itself, so that
 * hipEventElapsedTime(start, stop) is that kernel's own duration — what a kernel trace reports —
 * whatever the host's issue rate.  Consumed by that one launch; the brick pack and the fallback
 * launch are not bracketed.  Either event may be NULL. */
int sphrt_time_next_forward(void *start_event, void *stop_event);

/* ---- adjoint / back-projection (replaces Operator.T, raytracer.py:715-748, and the autograd
 * backward of raytracer.py:710) ------------------------------------------------------------ */
/* acc[c*chan_stride + vox[s]] += y[c*y_chan_stride + i] * len[s], float64 atomics into a zeroed
 * float64 accumulator `acc` (caller-allocated).  Same channel rules as forward. */
int sphrt_adjoint_accumulate(const sphrt_csr *csr, const void *y, int y_is_f64, int64_t n_chan,
                             int64_t y_chan_stride, int64_t ray_chan_div, double *acc,
                             int64_t chan_stride, void *stream);

/* Deterministic adjoint: the voxel-major transpose of the trace (built once).  col_ptr
 * (n_vox+1), t_ray / t_len (n_segments): for voxel v, the segments col_ptr[v] .. col_ptr[v+1]
 * in ray order (stable radix sort).  Index it with sphrt_csr_index(col_ptr, n_vox, t_ray, ...)
 * and the adjoint is sphrt_forward_f32/f64 on that CSR with y as the "density": no atomics,
 * bitwise reproducible. */
size_t sphrt_transpose_workspace_bytes(int64_t n_segments, int64_t n_vox);
int sphrt_csr_transpose(const sphrt_csr *csr, int64_t n_vox, int64_t *col_ptr, int32_t *t_ray,
                        double *t_len, void *workspace, size_t workspace_size, void *stream);
/* dst[i] = (float)src[i] — rounding the float64 accumulator to a float32 result. */
int sphrt_f64_to_f32(const double *src, float *dst, int64_t n, void *stream);
/* dst[i] = src[idx[i]], i < n (idx int32): the adjoint's input in trace order when the transposed
 * CSR's columns are trace rows (idx = the trace's ray ids), one launch instead of an
 * index_select. */
int sphrt_gather_f32(const float *src, const int32_t *idx, int64_t n, float *dst, void *stream);
int sphrt_gather_f64(const double *src, const int32_t *idx, int64_t n, double *dst, void *stream);

/* ---- retrieval loss tails (csrc/loss.hip; retrieval._gd_direct) ------------------------------
 * SquareLoss: r = yhat - y (y float32 or float64, promoted), r_scaled = r * scale, and the
 * partial sums of r * r; with `order` (NULL: identity), r_scaled[j] is ray order[j]'s (a
 * trace's sphrt_csr_index ray_ids: the transposed adjoint's input in trace order).  NegRegularizer: g -= c_neg where d < 0, and the partial sums of
 * |clamp(d, max=0)|.  The elementwise values are single IEEE operations, the values torch's
 * elementwise ops give (reference loss.py:87-162).  Each call writes sphrt_loss_partials(n)
 * partial sums (fixed partition and order); the loss is their sum / n, within rounding of
 * torch.mean. */
int64_t sphrt_loss_partials(int64_t n);
int sphrt_sq_residual_f64(const double *yhat, const void *y, int y_is_f64, int64_t n, double scale,
                          const int32_t *order, double *r_scaled, double *partial_sums,
                          void *stream);
/* sphrt_sq_residual_f64 with per-element factors, for SquareLoss(projection_mask=w) (reference
 * loss.py:87-110: lam * mean(w * (y - f(d))^2)).  With i = order ? order[j] : j:
 *   r           = yhat[i] - y[i]
 *   r_scaled[j] = r * ray_scale[i]
 *   partial sums of weight[i] * (r * r)      two roundings, the order torch's w * (y - f)**2 takes
 * ray_scale and weight are float64 arrays of n elements indexed as y is (through `order` when it
 * is given).  The same grid, the same sphrt_loss_partials(n) partial sums in the same fixed
 * order.  Fails on the host on n <= 0 and on a null yhat, y, ray_scale, weight, r_scaled or
 * partial_sums. */
int sphrt_wsq_residual_f64(const double *yhat, const void *y, int y_is_f64, int64_t n,
                           const double *ray_scale, const double *weight, const int32_t *order,
                           double *r_scaled, double *partial_sums, void *stream);
/* The robust residuals: psi of the residual in the residual's place (AbsLoss, reference
 * loss.py: lam * mean(w * |y - f(d)|); HuberLoss: lam * mean(w * huber_loss(f(d), y, delta))). */
#define SPHRT_RESID_ABS   1   /* psi(r) = sign(r): -1, 0, +1                      */
#define SPHRT_RESID_HUBER 2   /* psi(r) = r clamped to [-delta, delta], delta > 0  */
/* sphrt_wsq_residual_f64 for a robust loss: the same grid, the same sphrt_loss_partials(n)
 * partial sums in the same fixed order, the same use of `order`.  With i = order ? order[j] : j:
 *   r           = yhat[i] - y[i]                      one rounding (a float32 y promoted exactly)
 *   r_scaled[j] = psi(r) * ray_scale[i]               one rounding; exact for ABS
 *   ABS    partial sums of weight[i] * |r|            one rounding
 *   HUBER  partial sums of weight[i] * h(r), z = |r|,
 *          h = z < delta ? (0.5 * z) * z : delta * (z - 0.5 * delta)
 *                                                     torch's huber_loss forward, op by op
 * Every elementwise value is the one torch's elementwise ops give on the device (tested against
 * torch on an MI355X, tests/test_gpu_robust_gradient.py): sign(r) is (0 < r) - (r < 0), so a
 * residual of +-0 or NaN has psi = +0 under ABS — autograd's abs backward also gives a NaN
 * residual a zero gradient on the device, as on the CPU — and |NaN| = NaN in the sum; under HUBER
 * a NaN residual fails both compares, so psi, h and the sum are NaN, as torch's huber_loss
 * forward and backward give; +-inf is +-1 or +-delta with an infinite sum; denormals are not
 * flushed.  r_scaled is bitwise torch.sign(r) * ray_scale and torch.clamp(r, -delta, delta) *
 * ray_scale; against autograd's own chain the only difference is the sign of a zero under ABS
 * (autograd negates sign(y - f) * s, this forms sign(f - y) * s).  `delta` is unused for ABS.
 * Fails on the host on an unknown kind, for HUBER on a delta that is not finite and > 0, on
 * n <= 0 and on a null yhat, y, ray_scale, weight, r_scaled or partial_sums. */
int sphrt_robust_residual_f64(const double *yhat, const void *y, int y_is_f64, int64_t n,
                              int kind, double delta,
                              const double *ray_scale, const double *weight, const int32_t *order,
                              double *r_scaled, double *partial_sums, void *stream);
/* The Poisson fidelity's tail (PoissonLoss: lam * mean(w * (p - y * log(p + eps))), torch's
 * poisson_nll_loss(p, y, log_input=False, full=False, eps) under the mask): the grid, the use of
 * `order`, the sphrt_loss_partials(n) partial sums and their fixed order are
 * sphrt_robust_residual_f64's.  With i = order ? order[j] : j, p = yhat[i], s = ray_scale[i]:
 *   q           = p + eps                             one rounding (a float32 y promoted exactly)
 *   r_scaled[j] = s + ((-s) * y[i]) / q               a product, a quotient, a sum: three roundings
 *   partial sums of weight[i] * (p - y[i] * log(q))   the device's log, then three roundings
 * r_scaled[j] is the gradient autograd leaves at p for an incoming per-element gradient s —
 * the sub, mul and log backward of ATen's composite input - target * log(input + eps), in that
 * order — bitwise torch.autograd.grad's on the device, and the summed terms are bitwise torch's
 * own elementwise ones (both tested on an MI355X, tests/test_gpu_poisson_gradient.py).  Every
 * product is a plain multiply and the quotient a plain division, whatever -ffp-contract says.
 * There are no guards: q of +-0 gives -+inf or NaN, a negative q a NaN log, and inf and NaN
 * propagate, as in torch; denormals are not flushed.  Fails on the host, before any launch, on an
 * eps that is not finite and > 0, on n <= 0 and on a null yhat, y, ray_scale, weight, r_scaled or
 * partial_sums (`order` may be null). */
int sphrt_poisson_residual_f64(const double *yhat, const void *y, int y_is_f64, int64_t n,
                               double eps, const double *ray_scale, const double *weight,
                               const int32_t *order, double *r_scaled, double *partial_sums,
                               void *stream);
int sphrt_neg_reg_f64(const double *d, int64_t n, double c_neg, double *g, double *partial_sums,
                      void *stream);
/* SmoothRegularizer (loss.py; not in the reference): a difference penalty over the trailing axes
 * (t, r, e, a) of a contiguous float64 density of n_batch * nt * nr * ne * na = n voxels,
 *   P(d) = (1/N) * sum_ax w_ax * sum_{edges i -> i+1 along ax} rho(d[i+1] - d[i]),
 * rho(r) = r^2 (kind 0), |r| (SPHRT_RESID_ABS) or torch's huber_loss (SPHRT_RESID_HUBER, delta).
 * With wrap_a the edge from a = na - 1 to a = 0 closes every azimuth ring (na = 2: the pair is
 * joined by two edges).  An axis of length 1 or of weight 0 has no edges and is not read; no edge
 * crosses the batch axes (nt = 1: no time axis).  One launch writes
 *   g_out[i] = h_i, or g_in[i] + h_i when g_in is given
 *   G_i = (S_i * inv_n) * lam                                two roundings, in that order
 *   S_i = sum over the present neighbours, in the order t-, t+, r-, r+, e-, e+, a-, a+, of
 *         w_ax * rho'(d_i - d_nb),  rho' = 2r, sign(r) or clamp(r, +-delta)
 *   h_i = G_i, or with part_neg set G_i - c_neg where d_i < 0 (sphrt_neg_reg_f64's term, so that
 *         g_out = g_in + (G + neg): the order autograd leaves for [fidelity, two regularisers])
 * and the workgroup partial sums (sphrt_loss_partials(n) each, fixed partition and order) of
 * w_ax * rho(d[i+1] - d[i]) — every edge once, by its lower voxel; the wrap edge by the ring's
 * last voxel — into part_smooth, and with part_neg those of |clamp(d, max=0)|, as
 * sphrt_neg_reg_f64 leaves them.  The penalty is sum(part_smooth) * inv_n.  g_in may be NULL and
 * may be g_out; NaN and inf are not special-cased (they propagate as in the torch formula).
 * Fails on the host, before any launch, on an axis length < 1, n_batch < 1 (an empty volume),
 * n >= 2^31, a weight that is not finite and >= 0, a non-finite inv_n or lam, an unknown kind or
 * a HUBER delta that is not finite and > 0, a null part_smooth, g_out or d, and d == g_out. */
int sphrt_smooth_reg_f64(const double *d, int64_t n_batch, int nt, int nr, int ne, int na,
                         double wt, double wr, double we, double wa, int kind, double delta,
                         int wrap_a, double inv_n, double lam, double c_neg,
                         const double *g_in, double *g_out,
                         double *part_smooth, double *part_neg, void *stream);
/* One Adam step on float64 coefficients (torch.optim.Adam(fused=True), amsgrad and maximize off:
 * torch._fused_adam_'s per-element arithmetic, bitwise), step = the step count after this step's
 * increment (1, 2, ...).  With partial_sums set, the NegRegularizer is folded in first, as
 * sphrt_neg_reg_f64 on d = param before the step (grad itself is not modified); NULL: no
 * regulariser.  With stage_of (a brick-staged CSR over these n voxels, its `stage` buffer set),
 * the updated coefficients are also written to their staged columns, so the next forward can
 * run with stage_packed = 1 (pad columns are left as they are: zero after a forward's pack);
 * NULL: no stage.  Replaces, per retrieval iteration, the reference's optim.step() after
 * tot_loss.backward() (retrieval.py:115-116; loss.py:140-162 for the regulariser term). */
int sphrt_adam_neg_f64(double *param, const double *grad, double *exp_avg, double *exp_avg_sq,
                       int64_t n, double lr, double beta1, double beta2, double eps,
                       double weight_decay, double step, double c_neg, double *partial_sums,
                       const sphrt_csr *stage_of, void *stream);
/* The same step with the arithmetic of the default Adam on GPU tensors (torch.optim.Adam without
 * fused=: the multi-tensor "foreach" implementation, which the reference's optim(optim_vars,
 * **kwargs), retrieval.py:84, runs on a ROCm device), bitwise.  Its bias corrections come from
 * the host as torch computes them in Python: step_size = -lr / (1 - beta1**t), bc2_sqrt =
 * (1 - beta2**t) ** 0.5.  Regulariser and stage as sphrt_adam_neg_f64. */
int sphrt_adam_foreach_neg_f64(double *param, const double *grad, double *exp_avg,
                               double *exp_avg_sq, int64_t n, double step_size, double beta1,
                               double beta2, double eps, double weight_decay, double bc2_sqrt,
                               double c_neg, double *partial_sums, const sphrt_csr *stage_of,
                               void *stream);

/* ---- conjugate gradients: the vector side of an iteration (csrc/loss.hip; retrieval.cg) ------
 * For N x = b with N symmetric positive semi-definite, an iteration is h = N p (the operator's
 * entries and sphrt_smooth_reg_f64), then these three launches over the n elements of x, r, p, h
 * (float64, distinct buffers).  alpha and beta never reach the host: a launch leaves its
 * workgroups' partial sums of a dot product (the launch shape and partition of the entries
 * above), and the next launch has every workgroup sum those n_part <= 1024 partials itself in
 * one fixed order, so the scalar has the same bits in every workgroup:
 *   SUM(part): thread t of 256 adds part[t], part[t + 256], part[t + 512], part[t + 768] (those
 *   below n_part), in that order, onto +0.0; the 64 values of a wave by the xor butterfly 32,
 *   16, 8, 4, 2, 1 (v += v of lane ^ off; both lanes of a pair form the same sum); the four wave
 *   totals, in order, onto +0.0.
 * Every product feeding a sum is a plain multiply and every update one fma, whatever
 * -ffp-contract says; inf, NaN and denormals are not special-cased beyond the guards written
 * below (0 * inf is NaN, also with alpha = 0).  rr_stop points to one float64 on the device, the
 * squared residual norm at which the solve freezes; NULL: never.  Each entry fails on the host,
 * before any launch and without reading a pointer, on n <= 0, on a null buffer (rr_stop may be
 * NULL) and on n_part != the partial count of a launch over n elements.
 *
 *   h[i] = fma(c_damp, p[i], h[i]);  part_php: partial sums of p[i] * h[i] (the new h)        */
int sphrt_cg_curvature_f64(const double *p, double *h, int64_t n, double c_damp,
                           double *part_php, void *stream);
/*   RR = SUM(part_rr), PHP = SUM(part_php)
 *   alpha = (RR <= *rr_stop || !(PHP > 0) || !isfinite(RR / PHP)) ? 0 : RR / PHP
 *   x[i] = fma(alpha, p[i], x[i]);  r[i] = fma(-alpha, h[i], r[i])
 *   part_rr_new: partial sums of r[i] * r[i] (the new r); it may not be part_rr or part_php    */
int sphrt_cg_update_f64(double *x, double *r, const double *p, const double *h, int64_t n,
                        const double *part_rr, const double *part_php, int64_t n_part,
                        const double *rr_stop, double *part_rr_new, void *stream);
/*   RR_new = SUM(part_rr_new), RR_old = SUM(part_rr)
 *   beta = (RR_old <= *rr_stop || !(RR_old > 0)) ? 0 : RR_new / RR_old
 *   p[i] = fma(beta, p[i], r[i])                                                              */
int sphrt_cg_direction_f64(double *p, const double *r, int64_t n,
                           const double *part_rr_new, const double *part_rr, int64_t n_part,
                           const double *rr_stop, void *stream);

/* ---- projected gradient with momentum: the vector side of an iteration (retrieval.fista) ------
 * For min 1/2 x^T N x - b^T x subject to lower <= x <= upper, an iteration is g = N z - b without
 * the damping term (the operator's entries and sphrt_smooth_reg_f64), then these two launches
 * over the n elements of z, g, x_old, x_new (float64, distinct buffers), with the launch shape,
 * the partition, sphrt_loss_partials and SUM(part) of the entries above.  The step and the
 * restart decision never reach the host: `step` points to one float64 on the device (1 / L), and
 * the first launch leaves the partial sums the second one's workgroups sum themselves.  Every
 * product feeding a sum is a plain multiply and every update one fma; inf, NaN and denormals are
 * not special-cased (a NaN u fails both compares and stays NaN; a NaN GD does not restart).
 * lower / upper: -inf / +inf for no bound.  Each entry fails on the host, before any launch and
 * without reading a pointer, on n <= 0, a null buffer, buffers that overlap, n_part != the
 * partial count of a launch over n elements, n_omega < 2 and (the step entry) a NaN bound or
 * lower >= upper.
 *
 *   gp = fma(c_damp, z[i], g[i]);  u = fma(-*step, gp, z[i])
 *   x_new[i] = u < lower ? lower : (u > upper ? upper : u)
 *   part_gd: partial sums of gp * (x_new[i] - x_old[i]);  part_mm: of (z[i] - x_new[i])^2      */
int sphrt_pg_step_f64(const double *z, const double *g, const double *x_old, double *x_new,
                      int64_t n, double c_damp, const double *step, double lower, double upper,
                      double *part_gd, double *part_mm, void *stream);
/*   GD = SUM(part_gd);  j = GD > 0 ? 1 : min(*j_in + 1, n_omega - 1), and at least 0
 *   z[i] = fma(omega[j], x_new[i] - x_old[i], x_new[i]);  *j_out = j (thread 0 of workgroup 0,
 *   an ordinary store; j_in != j_out: consecutive slots of the caller's restart record)         */
int sphrt_pg_momentum_f64(double *z, const double *x_new, const double *x_old, int64_t n,
                          const double *part_gd, int64_t n_part, const double *omega,
                          int64_t n_omega, const int64_t *j_in, int64_t *j_out, void *stream);

/* ---- fused no-store mode: trace + integrate in one pass (nothing persisted) --------------- */
int sphrt_trace_integrate_f32(const sphrt_plan *plan, const sphrt_rays *rays,
                              const float *density, int64_t n_chan, int64_t chan_stride,
                              int64_t ray_chan_div, float *out, int64_t out_chan_stride,
                              void *workspace, size_t workspace_size, void *stream);
int sphrt_trace_integrate_f64(const sphrt_plan *plan, const sphrt_rays *rays,
                              const double *density, int64_t n_chan, int64_t chan_stride,
                              int64_t ray_chan_div, double *out, int64_t out_chan_stride,
                              void *workspace, size_t workspace_size, void *stream);
/* fused no-store adjoint: trace + scatter, nothing persisted.  acc as sphrt_adjoint_accumulate
 * (float64, zeroed and owned by the caller; float64 atomics, so sums are not bitwise
 * reproducible): acc[c*chan_stride + vox] += y[c*y_chan_stride + i] * len for every segment of
 * ray i, or with ray_chan_div > 0 (n_chan == 1) acc[(i / ray_chan_div)*chan_stride + vox] +=
 * y[i] * len.  Rays that miss the grid write nothing.  Fails on the host, before any launch, on a
 * null y or acc, a chan_stride below the grid's voxel count and a workspace smaller than
 * sphrt_trace_workspace_bytes.  Replaces Operator.T (raytracer.py:715-748) over a trace that is
 * never stored. */
int sphrt_trace_backproject_f64(const sphrt_plan *plan, const sphrt_rays *rays, const double *y,
                                int64_t n_chan, int64_t y_chan_stride, int64_t ray_chan_div,
                                double *acc, int64_t chan_stride,
                                void *workspace, size_t workspace_size, void *stream);
/* fused no-store least-squares gradient: one trace that integrates, forms the residual and
 * scatters it, nothing persisted.  For ray i and channel c (channels and time slices as
 * sphrt_trace_integrate_f64: density and acc channels chan_stride apart, m and yhat channels
 * y_chan_stride apart; with ray_chan_div > 0, n_chan == 1 and ray i reads and updates slice
 * i / ray_chan_div):
 *   yhat[c][i] = sum density[c][vox] * len        bitwise what sphrt_trace_integrate_f64 writes
 *   r          = (yhat[c][i] - m[c][i]) * scale   two roundings, as sphrt_sq_residual_f64
 *   acc[c][vox] += r * len                        for every segment of ray i (float64 atomics)
 * so acc receives A^T(scale * (A density - m)) and yhat A density.  acc is zeroed and owned by the
 * caller (sums are not bitwise reproducible); rays that miss the grid write yhat = 0 and add
 * nothing.  Fails on the host, before any launch, on a null plan or ray batch, a null density, m,
 * yhat or acc, n_chan < 1, ray_chan_div > 0 with n_chan != 1, a chan_stride below the grid's
 * voxel count, a y_chan_stride below the ray count when n_chan > 1, and a workspace smaller than
 * sphrt_trace_workspace_bytes.  Replaces Operator.__call__ plus Operator.T of the residual
 * (raytracer.py:692-748) over a trace that is never stored. */
int sphrt_trace_normal_f64(const sphrt_plan *plan, const sphrt_rays *rays,
                           const double *density, const double *m, double scale,
                           int64_t n_chan, int64_t chan_stride, int64_t ray_chan_div,
                           double *yhat, int64_t y_chan_stride,
                           double *acc, void *workspace, size_t workspace_size, void *stream);
/* Weighted least squares: sphrt_trace_normal_f64 with the scalar replaced by a factor per ray and
 * channel.  ray_scale is laid out exactly as m (channels y_chan_stride apart; with
 * ray_chan_div > 0 ray i's single value at i):
 *   yhat[c][i] = sum density[c][vox] * len                 bitwise sphrt_trace_integrate_f64's
 *   r          = (yhat[c][i] - m[c][i]) * ray_scale[c][i]  two roundings
 *   acc[c][vox] += r * len                                 one more, then a float64 atomic
 * so acc receives A^T(ray_scale .* (A density - m)).  The factor is read once per ray and
 * channel.  A ray whose factor is zero is traced and added like any other (its terms are +-0, or
 * NaN where its residual is not finite: NaN * 0 is NaN, as in torch).  Refusals as
 * sphrt_trace_normal_f64, and a null ray_scale; all on the host, before any launch. */
int sphrt_trace_normal_weighted_f64(const sphrt_plan *plan, const sphrt_rays *rays,
                                    const double *density, const double *m,
                                    const double *ray_scale,
                                    int64_t n_chan, int64_t chan_stride, int64_t ray_chan_div,
                                    double *yhat, int64_t y_chan_stride,
                                    double *acc, void *workspace, size_t workspace_size,
                                    void *stream);
/* Robust fidelity: sphrt_trace_normal_weighted_f64 with psi of the residual (SPHRT_RESID_*; the
 * sign for ABS, the clamp to +-delta for HUBER) in the residual's place:
 *   yhat[c][i] = sum density[c][vox] * len          bitwise sphrt_trace_integrate_f64's
 *   r          = yhat[c][i] - m[c][i]               one rounding
 *   w          = psi(r) * ray_scale[c][i]           one rounding; exact for ABS
 *   acc[c][vox] += w * len                          one more, then a float64 atomic
 * so acc receives A^T(ray_scale .* psi(A density - m)).  psi is sphrt_robust_residual_f64's,
 * special values included: a residual of +-0 (or, under ABS, NaN) has w = +-0 and adds nothing;
 * under HUBER a NaN residual adds NaN.  psi and the factor are formed once per ray and channel
 * (the lane-serial exact walk re-forms them per segment, as it re-reads the residual).
 * ray_scale is laid out as m and is always an array: a caller with one scalar expands it once.
 * Channels, ray_chan_div, a miss (yhat = 0, nothing added) and the workspace as the weighted
 * entry's.  `delta` is unused for ABS.  Refusals, all on the host before any launch: an unknown
 * kind, for HUBER a delta that is not finite and > 0, then sphrt_trace_normal_weighted_f64's. */
int sphrt_trace_normal_robust_f64(const sphrt_plan *plan, const sphrt_rays *rays,
                                  const double *density, const double *m,
                                  const double *ray_scale, int kind, double delta,
                                  int64_t n_chan, int64_t chan_stride, int64_t ray_chan_div,
                                  double *yhat, int64_t y_chan_stride,
                                  double *acc, void *workspace, size_t workspace_size,
                                  void *stream);
/* Poisson fidelity: sphrt_trace_normal_weighted_f64 with the Poisson weight in the scaled
 * residual's place.  It is not a function of the residual: it is formed from the sum and the
 * measurement separately, by sphrt_poisson_residual_f64's sequence:
 *   yhat[c][i] = sum density[c][vox] * len          bitwise sphrt_trace_integrate_f64's
 *   q          = yhat[c][i] + eps                   one rounding
 *   w          = s + ((-s) * m[c][i]) / q           s = ray_scale[c][i]; three roundings
 *   acc[c][vox] += w * len                          one more, then a float64 atomic
 * so acc receives A^T(ray_scale .* (1 - m / (A density + eps))), the gradient of
 * sum ray_scale .* (p - m log(p + eps)).  w is formed once per ray and channel (the lane-serial
 * exact walk re-forms it per segment, as it re-reads the sum).  No guards: q <= 0, inf and NaN
 * give what IEEE gives.  Channels, ray_chan_div, a miss (yhat = 0, nothing added) and the
 * workspace as the robust entry's.  Refusals, all on the host before any launch: an eps that is
 * not finite and > 0, then sphrt_trace_normal_weighted_f64's.
 * There is no fixed-point form: its bound needs max|w|, and |1 - m / (p + eps)| has no bound
 * before the forward has run.  The deterministic gradient is two traces over existing entries:
 * sphrt_trace_integrate_f64, sphrt_poisson_residual_f64, sphrt_fixed_scale_f64(a = r_scaled,
 * fa = L), sphrt_trace_backproject_fixed_f64, sphrt_fixed_finalize_f64. */
int sphrt_trace_normal_poisson_f64(const sphrt_plan *plan, const sphrt_rays *rays,
                                   const double *density, const double *m,
                                   const double *ray_scale, double eps,
                                   int64_t n_chan, int64_t chan_stride, int64_t ray_chan_div,
                                   double *yhat, int64_t y_chan_stride,
                                   double *acc, void *workspace, size_t workspace_size,
                                   void *stream);

/* ---- deterministic no-store adjoint: fixed-point scatter (csrc/fixed.hpp) --------------------
 * The two entries above sum y * len with float64 atomics, so their results differ in the last
 * bits from run to run.  The entries below quantise every term onto one power-of-two grid and
 * add it with integer atomics: integer addition is associative, so the result is bitwise
 * independent of the ray order, the workgroup schedule and the way a batch is split over calls.
 * The contract, exact on host and device:
 *   exponent  from a bound B >= |term| of every term (finite, > 0): frexp(B) = f * 2^E with f in
 *             [0.5, 1); the quantum is q = 2^(E - 61) (B is a rounded product: one bit of margin
 *             below int64's 63).
 *   quantise  k = llrint(ldexp(term, 61 - E)), round half to even; |k| <= 2^61.
 *   split     carry-save, no carry detection: element j of the accumulator owns the two adjacent
 *             int64 acc[2j] = lo and acc[2j + 1] = hi; lo += k & 0xffffffff, hi += k >> 32
 *             (arithmetic shift); its integer is V = hi * 2^32 + lo.  Both are plain integer
 *             sums, so accumulators filled under one record may be summed elementwise.
 *             Capacity: fewer than 2^31 adds per element over an accumulator's lifetime.
 *   value     ldexp(D, E - 61), D = V converted to double correctly rounded, ties to even.
 *   record    16 bytes of device memory, {int32 E, int32 flags, 8 bytes pad}.  flags bit 0: the
 *             bound was zero — nothing is added, every value is +0.0.  flags bit 1: the bound was
 *             not finite — nothing is added and EVERY value is NaN (the float64-atomic entries
 *             poison only the voxels the inf or NaN reaches; this way no host sync is needed).
 *
 * sphrt_fixed_scale_f64 (no counterpart above: the float64 sums need no scale) writes the record
 * of B = fa * max|a_i| + fb * max|b_j| (b NULL: the first term only), stream-ordered, no host
 * sync.  The maxima are taken over the bit patterns of |x| (a NaN sorts above infinity: the bound
 * is then not finite).  While it runs, the record's own 16 bytes hold the two maxima; the entry
 * resets them itself, the caller zeroes nothing.  For sphrt_trace_backproject_fixed_f64: a = y,
 * fa = L with L = 2 * r_b[nr], the outer sphere's diameter: no segment between two crossings of
 * a unit direction is longer.  (One kind is: the head segment of a start inside the grid runs
 * back to the farthest crossing behind the start, and directions shorter than 1 stretch every
 * length.  Terms above the bound are still quantised and added exactly, up to 2^32 times the
 * bound; each takes that many times more of the capacity, which is a bound on the sum of
 * |hi|: 2^63.)  For
 * sphrt_trace_normal_fixed_f64: a = density, fa = |scale| * L * L, b = m, fb = |scale| * L
 * (|yhat| <= max|density| * L).  Fails on the host on a null record, a negative length, a null
 * input of non-zero length and a negative or NaN factor. */
int sphrt_fixed_scale_f64(const double *a, int64_t na, double fa,
                          const double *b, int64_t nb, double fb,
                          void *scale_rec, void *stream);
/* Replaces sphrt_trace_backproject_f64 where the result must be reproducible: the same trace and
 * the same products y * len (one rounding each), then quantised under *scale_rec and added as two
 * 64-bit integer atomics.  acc holds 2 * n_chan * chan_stride int64 ({lo, hi} of element
 * c * chan_stride + vox), zeroed and owned by the caller; several calls may add into one acc
 * under one record (a batch split over calls gives the same bits as the whole).  Two integer
 * atomics per segment instead of one float64 atomic, 16 bytes per element instead of 8.  Fails on
 * the host, before any launch, as sphrt_trace_backproject_f64 does, and on a null scale record
 * and on n_rays * max(n_chan, 1) >= 2^29 (the capacity above). */
int sphrt_trace_backproject_fixed_f64(const sphrt_plan *plan, const sphrt_rays *rays,
                                      const double *y, int64_t n_chan, int64_t y_chan_stride,
                                      int64_t ray_chan_div, int64_t *acc, int64_t chan_stride,
                                      const void *scale_rec,
                                      void *workspace, size_t workspace_size, void *stream);
/* Replaces sphrt_trace_normal_f64 in the same way: yhat is bitwise the float64 forward, r the
 * same two roundings, r * len one more, then quantised and added as above.  acc, record,
 * refusals and cost as sphrt_trace_backproject_fixed_f64 (and sphrt_trace_normal_f64's own
 * refusals). */
int sphrt_trace_normal_fixed_f64(const sphrt_plan *plan, const sphrt_rays *rays,
                                 const double *density, const double *m, double scale,
                                 int64_t n_chan, int64_t chan_stride, int64_t ray_chan_div,
                                 double *yhat, int64_t y_chan_stride, int64_t *acc,
                                 const void *scale_rec,
                                 void *workspace, size_t workspace_size, void *stream);
/* Replaces sphrt_trace_normal_weighted_f64 in the same way: the same yhat, r and r * len, then
 * quantised under *scale_rec and added as two integer atomics.  The bound of its record:
 * sphrt_fixed_scale_f64(a = density, fa = S * L * L, b = m, fb = S * L) with S = max|ray_scale|
 * (the caller's to find; it must be finite) and L the outer diameter, since
 * |r * len| <= S * (max|density| * L + max|m|) * L.  acc, record, refusals and cost as
 * sphrt_trace_normal_fixed_f64, and a null ray_scale. */
int sphrt_trace_normal_weighted_fixed_f64(const sphrt_plan *plan, const sphrt_rays *rays,
                                          const double *density, const double *m,
                                          const double *ray_scale,
                                          int64_t n_chan, int64_t chan_stride,
                                          int64_t ray_chan_div,
                                          double *yhat, int64_t y_chan_stride, int64_t *acc,
                                          const void *scale_rec,
                                          void *workspace, size_t workspace_size, void *stream);
/* Replaces sphrt_trace_normal_robust_f64 in the same way: the same yhat, r, w and w * len, then
 * quantised under *scale_rec and added as two integer atomics.  The bound of its record needs no
 * host read of max|ray_scale|: sphrt_fixed_scale_f64(a = ray_scale, na, fa, b = NULL, 0, 0) with
 * fa = L for ABS and fa = delta * L for HUBER, L = 2 * r_b[nr] the outer diameter, since
 * |psi| <= 1 or delta and so |w * len| <= max|ray_scale| * fa (a ray_scale that is not finite
 * poisons the record: every value NaN).  As for the entries above, a head segment longer than L
 * is still quantised and added exactly, up to 2^32 times the bound.  acc, record, refusals and
 * cost as sphrt_trace_normal_weighted_fixed_f64, and sphrt_trace_normal_robust_f64's of kind and
 * delta. */
int sphrt_trace_normal_robust_fixed_f64(const sphrt_plan *plan, const sphrt_rays *rays,
                                        const double *density, const double *m,
                                        const double *ray_scale, int kind, double delta,
                                        int64_t n_chan, int64_t chan_stride,
                                        int64_t ray_chan_div,
                                        double *yhat, int64_t y_chan_stride, int64_t *acc,
                                        const void *scale_rec,
                                        void *workspace, size_t workspace_size, void *stream);
/* out[j] = the value of element j (acc[2j], acc[2j + 1]) under *scale_rec, one thread per
 * element; what reading the float64 accumulator of the entries it replaces was.  Fails on the
 * host on a null record, a negative n_elems and (n_elems > 0) a null acc or out. */
int sphrt_fixed_finalize_f64(const int64_t *acc, int64_t n_elems, const void *scale_rec,
                             double *out, void *stream);
/* acc element index[i] += terms[i] for i < n under *scale_rec, one thread per term: the device
 * quantise, split and two integer atomics of the trace entries above (the same device function),
 * on a caller's list of terms, so that the device arithmetic can be held to the host mirrors below
 * on chosen inputs.  Nothing is added when the record's flags are non-zero, as in the trace.
 * Every index[i] must name an element of acc (device memory: not checked).  Fails on the host on a
 * null record, a negative n and (n > 0) null terms, index or acc. */
int sphrt_fixed_accumulate_f64(const double *terms, const int64_t *index, int64_t n,
                               const void *scale_rec, int64_t *acc, void *stream);
/* Host-only mirrors of the arithmetic above (the same functions the kernels compile), for tests
 * and callers that need to predict bits.  sphrt_fixed_exponent_host: E and flags of a bound
 * (fails on a negative bound or a null output); sphrt_fixed_quantise_host: lo_hi = the split
 * quanta of one term; sphrt_fixed_value_host: the value of a {lo, hi} pair. */
int sphrt_fixed_exponent_host(double bound, int32_t *E, int32_t *flags);
void sphrt_fixed_quantise_host(double term, int32_t E, int64_t lo_hi[2]);
double sphrt_fixed_value_host(int64_t lo, int64_t hi, int32_t E, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* SPHRT_H */
