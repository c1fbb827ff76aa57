// fb_census.h -- the vortex census (fb_model_census, fb_slab_census): the 4-connected components of a thresholded field on the doubly
// periodic grid, labelled and measured on the GPU (definition: include/fftbaro.h; host side: fb_record.h, record_census).
//   k_census_init        label[c] = the first cell of c's run along j inside its aligned 64-cell segment (a wave's ballot), -1 off the mask
//   k_census_merge       union of every mask cell with its i+1 neighbour and, at a segment's end, its j+1 neighbour (both wrapped):
//                        the lock-free atomicMin union-find
//   k_census_flatten     label[c] = find(c), and the cells per root (int32 atomics, consecutive lanes of one root merged in the wave,
//                        the waves of a workgroup in LDS slots)
//   k_census_tile_counts, k_census_scan_tiles, k_census_ids
//                        a two-pass exclusive scan over the "kept root" flags: dense ids in label order, the same from call to call
//   k_census_sums        the moments of every kept structure with float64 atomics, the peak with one 64-bit atomicMax, combined in
//                        the wave and in LDS slots of the workgroup first
//   k_census_table       the peak unpacked, the unused rows filled
// Every array is indexed by the flat cell index ny i + j < nx ny <= 2^28.  The grids: nx and ny are multiples of 64, so a wave's 64
// consecutive cells (or a lane's four) never leave a row, and nx ny is a multiple of 4096, so every thread of a workgroup runs a
// grid-stride loop the same number of times (the wave operations inside are uniform).  No kernel waits for another workgroup.
// No reference counterpart.
#pragma once

enum { CENSUS_COLS = 12, CENSUS_TILE = 1024, CENSUS_SLOTS = 64 };
// the table's columns: 0 label  1 n  2 S_w  3 S_wx  4 S_wy  5 S_wxx  6 S_wyy  7 S_wxy  8 S_x  9 S_y  10 peak  11 peak_index
// (while k_census_sums runs, column 10 holds the packed peak key as 64 bits)

struct CensusGeo {
    double dx, dy;      // dx = Lx / nx, dy = Ly / ny from the context's float32 lengths widened
    int nx, ny;
    size_t n;           // nx ny
};

FB_DEV bool census_in(float f, float thr, int below) { return below ? f < thr : f > thr; }       // (a NaN compares false both ways)

// Every access to a label that another workgroup may be hooking is a relaxed agent-scope atomic: it reads the word where the
// atomicMin of any compute unit lands.  A label only ever decreases and is never negative on the mask, so every walk ends.
FB_DEV int census_load(const int *L, int x) { return __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
FB_DEV int census_find(const int *L, int x)
{
    for (;;) {
        const int p = census_load(L, x);
        if (p == x || p < 0) return x;
        x = p;
    }
}

// union of the trees of a and b: the larger root is hooked under the smaller.  atomicMin returns what the word held: the root
// itself -> hooked; anything else -> someone hooked it first, to `old`, and the word now holds min(old, b): the link to the larger of
// the two is gone (or was never made), so old and b remain to be united.  old < a: every retry follows a strictly smaller label.
FB_DEV void census_union(int *L, int a, int b)
{
    for (;;) {
        a = census_find(L, a);
        b = census_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(256) k_census_init(const float *__restrict__ f, float thr, int below, size_t n, int *__restrict__ label)
{
    const int lane = threadIdx.x & 63;
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
        const bool in = census_in(f[c], thr, below);
        const unsigned long long out_below = ~__ballot(in) & ((1ull << lane) - 1ull);   // the lanes below this one that are off the mask
        const int start = out_below ? 64 - __clzll((long long)out_below) : 0;           // the run starts right after the highest of them
        label[c] = in ? (int)(c - lane) + start : -1;
    }
}

// One cell per lane, a wave on 64 consecutive cells of a row.  Inside a segment a run is one tree already (k_census_init), so the
// j+1 union is due at a segment's last cell alone (the row's last cell wraps to its first), and the i+1 union of a cell whose left
// neighbour in the segment has the same two cells on the mask is implied by that neighbour's: the first cell of every stretch does it.
__global__ void __launch_bounds__(256) k_census_merge(CensusGeo g, int *label)
{
    const int lane = threadIdx.x & 63;
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < g.n; c += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(c / (size_t)g.ny), j = (int)(c - (size_t)i * g.ny);
        const size_t down = (size_t)(i + 1 == g.nx ? 0 : i + 1) * g.ny + j;
        const bool in = label[c] >= 0;                      // (the sign of a label never changes after k_census_init)
        const bool both = in && label[down] >= 0;
        const unsigned long long mb = __ballot(both);
        if (both && !(lane > 0 && ((mb >> (lane - 1)) & 1ull))) census_union(label, (int)c, (int)down);
        if (in && lane == 63) {
            const size_t right = j + 1 == g.ny ? c + 1 - g.ny : c + 1;
            if (label[right] >= 0) census_union(label, (int)c, (int)right);
        }
    }
}

// label[c] = its root, cnt[root] += 1 (cnt zeroed before).  Consecutive lanes of one root add once: the first lane of the stretch adds
// its length.  A large structure would still send every stretch of it to ONE word, and atomics on one address are served one after
// the other; so a workgroup first adds in LDS, in CENSUS_SLOTS slots taken by the first root that hashes there (a root that finds its
// slot taken by another adds to cnt directly), and adds the slots to cnt once per pass of its loop.
__global__ void __launch_bounds__(256) k_census_flatten(size_t n, int *label, int *__restrict__ cnt)
{
    __shared__ int s_root[CENSUS_SLOTS], s_cnt[CENSUS_SLOTS];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < CENSUS_SLOTS) { s_root[threadIdx.x] = -1; s_cnt[threadIdx.x] = 0; }
    __syncthreads();
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
        int r = label[c];
        if (r >= 0) { r = census_find(label, (int)c); label[c] = r; }
        const int prev = __shfl_up(r, 1);
        const bool head = lane == 0 || prev != r;
        const unsigned long long heads = __ballot(head);    // (by every lane: inside the conditional below lane 63 would not vote)
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);               // the heads above this lane
        if (head && r >= 0) {
            const int len = above ? __ffsll((long long)above) : 64 - lane, h = r & (CENSUS_SLOTS - 1);
            const int own = atomicCAS(&s_root[h], -1, r);
            if (own == -1 || own == r) atomicAdd(&s_cnt[h], len);
            else atomicAdd(cnt + r, len);
        }
        __syncthreads();
        if (threadIdx.x < CENSUS_SLOTS && s_root[threadIdx.x] >= 0) {
            atomicAdd(cnt + s_root[threadIdx.x], s_cnt[threadIdx.x]);
            s_root[threadIdx.x] = -1; s_cnt[threadIdx.x] = 0;
        }
        __syncthreads();
    }
}

// the flags of a lane's four cells: bit k of `root`: cell 4 e + k is a root; of `kept`: a root of at least min_cells cells
FB_DEV void census_flags(const int *label, const int *cnt, size_t e, int min_cells, int &root, int &kept)
{
    const int4 l = *reinterpret_cast<const int4 *>(label + 4 * e), q = *reinterpret_cast<const int4 *>(cnt + 4 * e);
    const int la[4] = {l.x, l.y, l.z, l.w}, qa[4] = {q.x, q.y, q.z, q.w};
    root = kept = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (la[k] == (int)(4 * e) + k) { root |= 1 << k; if (qa[k] >= min_cells) kept |= 1 << k; }
}

// a workgroup of 256 per tile of CENSUS_TILE cells: part[tile] = (kept roots, roots)
__global__ void __launch_bounds__(256) k_census_tile_counts(const int *__restrict__ label, const int *__restrict__ cnt, int ntiles, int min_cells, int2 *__restrict__ part)
{
    __shared__ int sk[4], sr[4];
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int root, kept;
        census_flags(label, cnt, (size_t)t * 256 + threadIdx.x, min_cells, root, kept);
        int nk = __popc(kept), nr = __popc(root);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { nk += __shfl_xor(nk, o); nr += __shfl_xor(nr, o); }
        if ((threadIdx.x & 63) == 0) { sk[threadIdx.x >> 6] = nk; sr[threadIdx.x >> 6] = nr; }
        __syncthreads();
        if (threadIdx.x == 0) part[t] = make_int2(sk[0] + sk[1] + sk[2] + sk[3], sr[0] + sr[1] + sr[2] + sr[3]);
        __syncthreads();
    }
}

// one workgroup of 1024: part[t].x -> the kept roots of the tiles before t; count[0] = the kept structures, count[1] = all.  A thread
// takes a stretch of consecutive tiles; the stretches' sums are scanned in LDS.
__global__ void __launch_bounds__(1024) k_census_scan_tiles(int2 *__restrict__ part, int ntiles, int *__restrict__ count)
{
    __shared__ int sk[1024], sr[1024];
    const int per = (ntiles + 1023) / 1024, t0 = min((int)threadIdx.x * per, ntiles), t1 = min(t0 + per, ntiles);
    int nk = 0, nr = 0;
    for (int t = t0; t < t1; ++t) { nk += part[t].x; nr += part[t].y; }
    sk[threadIdx.x] = nk; sr[threadIdx.x] = nr;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                    // inclusive scans
        const bool up = threadIdx.x >= (unsigned)o;
        const int a = up ? sk[threadIdx.x - o] : 0, b = up ? sr[threadIdx.x - o] : 0;
        __syncthreads();
        sk[threadIdx.x] += a; sr[threadIdx.x] += b;
        __syncthreads();
    }
    int run = sk[threadIdx.x] - nk;
    for (int t = t0; t < t1; ++t) { const int k = part[t].x; part[t].x = run; run += k; }
    if (threadIdx.x == 1023) { count[0] = sk[1023]; count[1] = sr[1023]; }
}

// per tile: the dense id of every kept root = the tile's offset + the kept roots before it in the tile; cnt[root] = that id, or -1 for
// a dropped root (the counts have done their work); the label column of the table's row
__global__ void __launch_bounds__(256) k_census_ids(const int *__restrict__ label, int *__restrict__ cnt, const int2 *__restrict__ part, int ntiles, int min_cells,
                                                    int max_structures, double *__restrict__ table)
{
    __shared__ int sw[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const size_t e = (size_t)t * 256 + threadIdx.x;
        int root, kept;
        census_flags(label, cnt, e, min_cells, root, kept);
        const int mine = __popc(kept);
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (lane >= o) incl += v; }
        if (lane == 63) sw[w] = incl;
        __syncthreads();
        int id = part[t].x + incl - mine;
        for (int q = 0; q < w; ++q) id += sw[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!((root >> k) & 1)) continue;
            const size_t c = 4 * e + k;
            if ((kept >> k) & 1) {
                cnt[c] = id;
                if (id < max_structures) table[(size_t)id * CENSUS_COLS] = (double)c;
                ++id;
            } else cnt[c] = -1;
        }
        __syncthreads();
    }
}

// the sums of one run of cells of one structure, and the packed key of its peak
struct CensusRun {
    double s[9];                // n, S_w, S_wx, S_wy, S_wxx, S_wyy, S_wxy, S_x, S_y
    unsigned long long key;     // bits(|w|) high, ~index low: the largest |w|, ties to the smallest index; 0: no cell compared
};

// the workgroup's LDS slots of k_census_sums: the id that took the slot (-1: free), its sums and its key
struct CensusSlots {
    int id[CENSUS_SLOTS];
    double s[CENSUS_SLOTS][9];
    unsigned long long key[CENSUS_SLOTS];
};

FB_DEV void census_to_table(int id, const double *s, unsigned long long key, double *table)
{
    double *row = table + (size_t)id * CENSUS_COLS;
#pragma unroll
    for (int k = 0; k < 9; ++k) unsafeAtomicAdd(row + 1 + k, s[k]);
    if (key) atomicMax(reinterpret_cast<unsigned long long *>(row + 10), key);
}

// a run of structure `id` into the workgroup's slot where the id holds it (or takes it), else straight to the table
FB_DEV void census_flush(int id, const CensusRun &r, int max_structures, double *table, CensusSlots &S)
{
    if (id < 0 || id >= max_structures) return;
    const int h = id & (CENSUS_SLOTS - 1);
    const int own = atomicCAS(&S.id[h], -1, id);
    if (own != -1 && own != id) { census_to_table(id, r.s, r.key, table); return; }
#pragma unroll
    for (int k = 0; k < 9; ++k) __hip_atomic_fetch_add(&S.s[h][k], r.s[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (r.key) __hip_atomic_fetch_max(&S.key[h], r.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

FB_DEV void census_slots_clear(CensusSlots &S)
{
    if (threadIdx.x < CENSUS_SLOTS) {
        S.id[threadIdx.x] = -1; S.key[threadIdx.x] = 0ull;
#pragma unroll
        for (int k = 0; k < 9; ++k) S.s[threadIdx.x][k] = 0.0;
    }
}

// A lane takes four neighbouring cells of a row and keeps a run (id, sums) in registers, flushed to the table when the id changes.
// The last run of every lane is first added up over the consecutive lanes of the wave that hold the same id (a structure wider than
// four cells spans lanes), and the first lane of such a stretch adds the stretch to the table: float64 atomic adds, and one 64-bit
// atomicMax for the peak -- through the workgroup's LDS slots (CensusSlots), which go to the table once per pass of the loop: a large
// structure on a speckled mask would otherwise arrive as millions of adds on one row, served one after the other.  ids: the dense id per root (k_census_ids).  V4: w and d_ids are 16-byte aligned.  d_ids (may be NULL): the id map.
template <bool V4>
__global__ void __launch_bounds__(256) k_census_sums(CensusGeo g, const int *__restrict__ label, const int *__restrict__ ids, const float *__restrict__ w,
                                                     int max_structures, double *__restrict__ table, int *__restrict__ d_ids)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int hx = g.nx / 2, hy = g.ny / 2;
    __shared__ CensusSlots S;
    census_slots_clear(S);
    __syncthreads();
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < g.n / 4; e += (size_t)gridDim.x * blockDim.x) {
        const size_t c0 = 4 * e;
        const int i = (int)(c0 / (size_t)g.ny), j = (int)(c0 - (size_t)i * g.ny);
        const int4 l4 = *reinterpret_cast<const int4 *>(label + c0);
        const int la[4] = {l4.x, l4.y, l4.z, l4.w};
        float wa[4];
        if (V4) { const float4 w4 = *reinterpret_cast<const float4 *>(w + c0); wa[0] = w4.x; wa[1] = w4.y; wa[2] = w4.z; wa[3] = w4.w; }
        else { wa[0] = w[c0]; wa[1] = w[c0 + 1]; wa[2] = w[c0 + 2]; wa[3] = w[c0 + 3]; }
        int ida[4];
        int cur = -1, cur_label = -1;
        CensusRun r;
#pragma unroll
        for (int q = 0; q < 9; ++q) r.s[q] = 0.0;
        r.key = 0ull;
        double ex = 0.0;
        int j0 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int L = la[k];
            const int id = L < 0 ? -1 : (L == cur_label ? cur : ids[L]);
            ida[k] = id;
            if (L != cur_label) {
                census_flush(cur, r, max_structures, table, S);
                cur = id; cur_label = L;
#pragma unroll
                for (int q = 0; q < 9; ++q) r.s[q] = 0.0;
                r.key = 0ull;
                if (id >= 0) {
                    const int i0 = L / g.ny;
                    j0 = L - i0 * g.ny;
                    ex = (double)((i - i0 + hx + g.nx) % g.nx - hx) * g.dx;
                }
            }
            if (id < 0) continue;
            const double ey = (double)((j + k - j0 + hy + g.ny) % g.ny - hy) * g.dy;
            const double wd = (double)wa[k], wx = wd * ex, wy = wd * ey;
            r.s[0] += 1.0; r.s[1] += wd; r.s[2] += wx; r.s[3] += wy; r.s[4] += wx * ex; r.s[5] += wy * ey; r.s[6] += wx * ey; r.s[7] += ex; r.s[8] += ey;
            if (wa[k] == wa[k]) {
                const unsigned long long key = ((unsigned long long)(__float_as_uint(wa[k]) & 0x7fffffffu) << 32) | (unsigned)~(unsigned)(c0 + k);
                if (key > r.key) r.key = key;
            }
        }
        if (d_ids) {
            if (V4) *reinterpret_cast<int4 *>(d_ids + c0) = make_int4(ida[0], ida[1], ida[2], ida[3]);
            else { d_ids[c0] = ida[0]; d_ids[c0 + 1] = ida[1]; d_ids[c0 + 2] = ida[2]; d_ids[c0 + 3] = ida[3]; }
        }
        // the stretch of lanes whose last run has this lane's id: [its head, end)
        const int prev = __shfl_up(cur, 1);
        const bool head = lane == 0 || prev != cur;
        const unsigned long long heads = __ballot(head);    // (by every lane, as in k_census_flatten)
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int end = above ? lane + __ffsll((long long)above) : 64;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const bool take = lane + o < end;
#pragma unroll
            for (int q = 0; q < 9; ++q) { const double v = __shfl_down(r.s[q], o); if (take) r.s[q] += v; }
            const unsigned long long kk = __shfl_down(r.key, o);
            if (take && kk > r.key) r.key = kk;
        }
        if (head) census_flush(cur, r, max_structures, table, S);
        __syncthreads();
        if (threadIdx.x < CENSUS_SLOTS && S.id[threadIdx.x] >= 0) census_to_table(S.id[threadIdx.x], S.s[threadIdx.x], S.key[threadIdx.x], table);
        __syncthreads();
        census_slots_clear(S);
        __syncthreads();
    }
}

// one thread per row of the table: the rows of the structures found get peak and peak_index from the key (the peak's sign from w
// itself; a structure whose every w is a NaN: NaN and -1), the rows from min(found, max_structures) on label -1 and zeros
__global__ void __launch_bounds__(256) k_census_table(const int *__restrict__ count, const float *__restrict__ w, int max_structures, double *__restrict__ table)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= max_structures) return;
    double *row = table + (size_t)r * CENSUS_COLS;
    if (r < count[0]) {
        const unsigned long long key = *reinterpret_cast<const unsigned long long *>(row + 10);
        const unsigned at = ~(unsigned)key;
        row[10] = key ? (double)w[at] : __builtin_nan("");
        row[11] = key ? (double)at : -1.0;
    } else {
        row[0] = -1.0;
#pragma unroll
        for (int k = 1; k < CENSUS_COLS; ++k) row[k] = 0.0;
    }
}
