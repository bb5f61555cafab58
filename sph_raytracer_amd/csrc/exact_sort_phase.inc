// exact_sort_phase.inc — the sort phase of the wave-parallel introsort emulation (trace.hip): the
// partitions (the top levels breadth-first over the W waves, then each wave its range depth-first
// with its LDS stack; depth-limit ranges through exact_heap_range), then the final insertion sort
// as ranks inside each leaf.  The list (tk, pk) in concatenation order, NaN-free, with leaf[] and
// top[] initialised and synced -> (ts, ps) in the reference's order, synced.
//
// Program text, included where these names are in scope: INV, W; v, tk, pk, ts, ps, lpos, rpos,
// leaf, st_first, st_last, st_depth, top; K, r_lim, e_lim, s, tid, lane, wid, below, n_heap.
// exact_wave_kernel includes it in place and exact_wave_sort wraps it for the test hook: as a
// function called from the kernel the same text costs every one-wave instantiation two VGPRs
// (and three of them a wave of occupancy); included, the kernels compile as before.
    // ---- partition phase (uniform control flow per wave) ----
    // the top levels, breadth-first: range w of level l splits into ranges w and w + 2^l
#pragma unroll
    for (int n = 1; n < W; n *= 2) {
        if (wid < n) {
            const int f = top[3 * wid], l = top[3 * wid + 1], dep = top[3 * wid + 2];
            int cut = l, nd = dep;
            if (l - f > kIntroThreshold && dep > 0) {
                cut = exact_partition(v, tk, pk, lpos, rpos, f, l, lane, below);
                nd = dep - 1;
            }
            if (lane == 0) {
                top[3 * wid + 1] = cut;
                top[3 * wid + 2] = nd;
                top[3 * (wid + n)] = cut;
                top[3 * (wid + n) + 1] = l;
                top[3 * (wid + n) + 2] = nd;
            }
        }
        __syncthreads();
    }
    // then each wave its range, depth first
    int sp = 0;
    int first = top[3 * wid], last = top[3 * wid + 1], depth = top[3 * wid + 2];
    bool have = last - first > 1;
    while (have) {
        while (last - first > kIntroThreshold) {
            if (depth == 0) {                      // the reference's heapsort
                exact_heap_range<INV>(v, tk, pk, ts, ps, lpos, first, last, K, r_lim, e_lim, s,
                                      lane, n_heap);
                first = last;                      // sorted: no leaf
                break;
            }
            --depth;
            const int cut = exact_partition(v, tk, pk, lpos, rpos, first, last, lane, below);
            if (lane == 0) {
                st_first[sp] = cut;
                st_last[sp] = last;
                st_depth[sp] = depth;
            }
            ++sp;
            last = cut;
            wave_sync();
        }
        if (last - first > 1) {                    // a leaf: its range, for the final ranks
            const uint32_t code = (uint32_t)first | ((uint32_t)last << 16);
            for (int p = first + lane; p < last; p += 64) leaf[p] = code;
        }
        have = sp > 0;
        if (have) {
            --sp;
            first = st_first[sp];
            last = st_last[sp];
            depth = st_depth[sp];
        }
    }
    __syncthreads();
    // ---- final insertion sort = stable sort inside each leaf, as ranks ----
    for (int p = tid; p < K; p += 64 * W) {
        const uint32_t code = leaf[p];
        const int lo = (int)(code & 0xffffu), hi = (int)(code >> 16);
        const double t = tk[p];
        int r = lo;
        for (int j = lo; j < hi; ++j) {
            const double u = tk[j];
            r += (u < t || (u == t && j < p)) ? 1 : 0;
        }
        ts[r] = t;
        ps[r] = pk[p];
    }
    __syncthreads();
