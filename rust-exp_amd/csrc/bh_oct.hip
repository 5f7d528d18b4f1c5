// bh_oct.hip -- the octree of the 3-D Barnes-Hut path (NBX_OPT_BH_DIM = 3), built on the device.  COMPILED WITH -ffp-contract=off.
//
// The reference (rs-src/nbody.rs) is planar; this is its tree with z added, rule for rule:
//   * root box = the per-axis AABB of the bodies (nbody.rs:388-398 plus z), not made cubic;
//   * a node is split iff it holds two bodies that do not share a level-21 cell; child boxes from midpoints (a1 + a2) * 0.5 in
//     unfused f32 (nbody.rs:289-300); child index 4 (z < cz) + 2 (y < cy) + (x >= cx) -- the reference's UL, UR, LL, LR with z as
//     the slow digit, so a system with z == 0 everywhere (cz == z: always the upper half) builds today's quadtree node for node;
//   * empty children are dropped, single-child chain nodes exist, as in the reference;
//   * 21 levels (63-bit keys).  Bodies that share a level-21 cell form ONE leaf (summed mass, centre of mass): this stands in for
//     the reference's EPS merge (nbody.rs:249-260) -- with a root box up to the kill box (110 wide) such a cell is 5e-5 wide,
//     below EPS.  A leaf whose bodies are NOT within EPS of each other on every axis (a huge root box) raises counters[2]: the
//     caller reports NBX_ERR_TREE_DEPTH, the analogue of the reference's depth panic (nbody.rs:230-232).
//     OUT OF SCOPE: the arrival-order replay of EPS chains across cells that the quadtree build has (bh_build.hip k_chain*).
//   * an interior node's (px, py, pz, m) = f32 roundings of fp64 sums over its bodies; a single-body leaf = the body unchanged.
//
// One pass per step, cold every step ("the tree from the sorted keys", bh_build_internal.h, with 3-bit digits):
//   k_oct_bbox     six-component AABB partials (at most 256), folded by every workgroup of the next kernel
//   k_oct_keys     21 replayed three-axis descents per body -> (key, body index)
//   rocPRIM        radix sort of the pairs over 63 bits (the only library call)
//   k_oct_scan_*   cnt(a) = leaf(a) - c(a) nodes start at sorted body a, leaf(a) = min(21, 1 + max(c(a), c(a+1))); fp64 prefix sums
//                  of m, m x, m y, m z; exclusive scans of node and leaf counts.  The host reads the counts (one small
//                  synchronous read per step) and sizes the node and group arrays from them.
//   k_oct_emit     one thread per node: owner body by a search of the scanned counts, body range by galloping over the keys,
//                  centre from prefix differences (direct sums up to 8 bodies), s by replaying the x-descent along the key
#include <cstring>   // rocPRIM's texture_cache_iterator.hpp calls memset() without including it

#include <rocprim/device/device_radix_sort.hpp>

#include "kernels.h"

namespace nbx {

typedef unsigned long long u64;
constexpr int kOctScanPerThread = 4;
constexpr int kOctScanBlock = kTile * kOctScanPerThread;
constexpr int kOctParts = 256;

struct OctScan {
    double m, mx, my, mz;
    int cnt;   // nodes starting at the body
    int ent;   // 1 if the body starts a leaf (i.e. any node at all)
};
__device__ __forceinline__ OctScan oct_add(const OctScan& a, const OctScan& b)
{
    return OctScan{a.m + b.m, a.mx + b.mx, a.my + b.my, a.mz + b.mz, a.cnt + b.cnt, a.ent + b.ent};
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------
// header: ints [0] nodes [1] leaves [2] leaves wider than EPS [3] depth, floats [8..13] the root box (x1 y1 z1 x2 y2 z2)
struct OctWs {
    int* counters;
    float* box;
    float4* part;                 // [2 * kOctParts] (min, max) partial boxes
    u64 *keys0, *keys1;
    unsigned *idx0, *idx1;
    void* sort_tmp;
    float4* sb;                   // bodies in key order
    double *pm, *pmx, *pmy, *pmz; // [n + 1] exclusive prefix sums over the sorted bodies
    int* base;                    // [n + 1] pre-order slot of the first node starting at body j; base[n] = number of nodes
    int* ent;                     // [n + 1] leaves that start before body j
    unsigned char* cnt;           // [n] nodes starting at body j
    OctScan* block_sums;          // [nb + 1]
};
static OctWs oct_carve(void* workspace, int n, size_t sort_tmp, size_t* total = nullptr)
{
    char* w = static_cast<char*>(workspace);
    auto take = [&](size_t b) { char* p = w; w += (b + 255) & ~(size_t)255; return p; };
    const size_t nb = ((size_t)n + kOctScanBlock - 1) / kOctScanBlock;
    OctWs k;
    char* header = take(256);
    k.counters = reinterpret_cast<int*>(header);
    k.box = reinterpret_cast<float*>(header) + 8;
    k.part = reinterpret_cast<float4*>(take(sizeof(float4) * 2 * kOctParts));
    k.keys0 = reinterpret_cast<u64*>(take(sizeof(u64) * (size_t)n));
    k.keys1 = reinterpret_cast<u64*>(take(sizeof(u64) * (size_t)n));
    k.idx0 = reinterpret_cast<unsigned*>(take(sizeof(unsigned) * (size_t)n));
    k.idx1 = reinterpret_cast<unsigned*>(take(sizeof(unsigned) * (size_t)n));
    k.sort_tmp = take(sort_tmp);
    k.sb = reinterpret_cast<float4*>(take(sizeof(float4) * (size_t)n));
    k.pm = reinterpret_cast<double*>(take(sizeof(double) * ((size_t)n + 1)));
    k.pmx = reinterpret_cast<double*>(take(sizeof(double) * ((size_t)n + 1)));
    k.pmy = reinterpret_cast<double*>(take(sizeof(double) * ((size_t)n + 1)));
    k.pmz = reinterpret_cast<double*>(take(sizeof(double) * ((size_t)n + 1)));
    k.base = reinterpret_cast<int*>(take(sizeof(int) * ((size_t)n + 1)));
    k.ent = reinterpret_cast<int*>(take(sizeof(int) * ((size_t)n + 1)));
    k.cnt = reinterpret_cast<unsigned char*>(take((size_t)n));
    k.block_sums = reinterpret_cast<OctScan*>(take(sizeof(OctScan) * (nb + 1)));
    if (total) *total = (size_t)(w - static_cast<char*>(workspace));
    return k;
}

size_t oct_workspace_bytes(int n, size_t* sort_tmp_bytes)
{
    thread_local int memo_n = -1;   // (the size query is host work inside the library: asked once per n)
    thread_local size_t memo_tmp = 0;
    if (n != memo_n) {
        size_t tmp = 0;
        (void)rocprim::radix_sort_pairs(nullptr, tmp, (u64*)nullptr, (u64*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, (size_t)n, 0,
                                        3 * kOctLevels, (hipStream_t)0);
        memo_n = n;
        memo_tmp = tmp;
    }
    if (sort_tmp_bytes) *sort_tmp_bytes = memo_tmp;
    size_t total = 0;
    (void)oct_carve(nullptr, n, memo_tmp, &total);
    return total;
}
const int* oct_counters(const void* workspace) { return static_cast<const int*>(workspace); }
const unsigned* oct_order(void* workspace, int n, size_t sort_tmp_bytes) { return oct_carve(workspace, n, sort_tmp_bytes).idx1; }

// ---- root box and keys -------------------------------------------------------------------------------------------------------
constexpr float kBig = 3.40282347e+38f;

__device__ __forceinline__ void oct_wave_minmax(float (&lo)[3], float (&hi)[3])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
        }
}
// collective over a workgroup of kTile threads: every thread leaves with the fold of all threads' boxes
__device__ __forceinline__ void oct_block_minmax(float (&lo)[3], float (&hi)[3])
{
    __shared__ float red[kTile / 64][6];
    oct_wave_minmax(lo, hi);
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; a++) { red[threadIdx.x >> 6][a] = lo[a]; red[threadIdx.x >> 6][3 + a] = hi[a]; }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = red[0][a]; hi[a] = red[0][3 + a];
        for (int w = 1; w < kTile / 64; w++) { lo[a] = fminf(lo[a], red[w][a]); hi[a] = fmaxf(hi[a], red[w][3 + a]); }
    }
}

__global__ __launch_bounds__(kTile) void k_oct_bbox(const float4* __restrict__ posm, const int n, float4* __restrict__ part,
                                                    int* __restrict__ counters)
{
    if (blockIdx.x == 0 && threadIdx.x < 4) counters[threadIdx.x] = 0;   // this build's counters (the kernels behind add to them)
    float lo[3] = {kBig, kBig, kBig}, hi[3] = {-kBig, -kBig, -kBig};
    for (int i = blockIdx.x * kTile + threadIdx.x; i < n; i += (int)gridDim.x * kTile) {
        const float4 q = posm[i];
        lo[0] = fminf(lo[0], q.x); lo[1] = fminf(lo[1], q.y); lo[2] = fminf(lo[2], q.z);
        hi[0] = fmaxf(hi[0], q.x); hi[1] = fmaxf(hi[1], q.y); hi[2] = fmaxf(hi[2], q.z);
    }
    oct_block_minmax(lo, hi);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x + 0] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        part[2 * blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// one step of the reference's quadrant_from_point + create_children (nbody.rs:289-300,:324-331) on three axes
__device__ __forceinline__ int oct_descend(float (&lo)[3], float (&hi)[3], const float x, const float y, const float z)
{
    const float cx = __fmul_rn(__fadd_rn(lo[0], hi[0]), 0.5f);
    const float cy = __fmul_rn(__fadd_rn(lo[1], hi[1]), 0.5f);
    const float cz = __fmul_rn(__fadd_rn(lo[2], hi[2]), 0.5f);
    int q = 0;
    if (z < cz) { q = 4; hi[2] = cz; } else { lo[2] = cz; }
    if (y < cy) { q += 2; hi[1] = cy; } else { lo[1] = cy; }
    if (x < cx) { hi[0] = cx; } else { q += 1; lo[0] = cx; }
    return q;
}

__global__ __launch_bounds__(kTile) void k_oct_keys(const float4* __restrict__ posm, const int n, const float4* __restrict__ part,
                                                    const int parts, float* __restrict__ box, u64* __restrict__ keys,
                                                    unsigned* __restrict__ idx)
{
    float lo[3] = {kBig, kBig, kBig}, hi[3] = {-kBig, -kBig, -kBig};
    if ((int)threadIdx.x < parts) {   // (parts <= kOctParts = kTile; min and max are exact in any order: who folds changes no bit)
        const float4 a = part[2 * threadIdx.x], b = part[2 * threadIdx.x + 1];
        lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = b.x; hi[1] = b.y; hi[2] = b.z;
    }
    oct_block_minmax(lo, hi);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int a = 0; a < 3; a++) { box[a] = lo[a]; box[3 + a] = hi[a]; }
    const int i = blockIdx.x * kTile + threadIdx.x;
    if (i >= n) return;
    const float4 p = posm[i];
    u64 key = 0;
#pragma unroll 1
    for (int l = 0; l < kOctLevels; l++) key = (key << 3) | (u64)oct_descend(lo, hi, p.x, p.y, p.z);
    keys[i] = key;
    idx[i] = (unsigned)i;
}

// ---- the tree from the sorted keys ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int oct_common(const u64 x, const u64 y)
{
    const u64 d = x ^ y;
    if (d == 0ull) return kOctLevels;
    return (__clzll((long long)d) - 1) / 3;   // keys occupy the low 63 bits, digit l = bits 62-3l .. 60-3l
}
// do the keys share their first `depth` digits?
__device__ __forceinline__ bool oct_same_prefix(const u64 x, const u64 y, const int depth)
{
    return depth == 0 || ((x ^ y) >> (3 * (kOctLevels - depth))) == 0ull;
}
// first index > a whose key does not share the first `depth` digits of keys[a] (n if none)
__device__ __forceinline__ int oct_range_end(const u64* __restrict__ keys, const int a, const int n, const int depth)
{
    const u64 k = keys[a];
    int lo = a, step = 1;
    while (lo + step < n && oct_same_prefix(keys[lo + step], k, depth)) { lo += step; step <<= 1; }
    int hi = lo + step < n ? lo + step : n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (oct_same_prefix(keys[mid], k, depth)) lo = mid; else hi = mid;
    }
    return hi;
}

// collective over a workgroup of kTile threads: exclusive prefix of v in thread order; total = the sum over the workgroup
__device__ __forceinline__ OctScan oct_shfl_up(const OctScan& a, const int d)
{
    return OctScan{__shfl_up(a.m, d), __shfl_up(a.mx, d), __shfl_up(a.my, d), __shfl_up(a.mz, d), __shfl_up(a.cnt, d), __shfl_up(a.ent, d)};
}
__device__ __forceinline__ OctScan oct_block_exclusive(const OctScan v, OctScan& total)
{
    __shared__ OctScan wsum[kTile / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    OctScan inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const OctScan o = oct_shfl_up(inc, d);
        if (lane >= d) inc = oct_add(o, inc);
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    OctScan prev = oct_shfl_up(inc, 1);
    const OctScan zero{0.0, 0.0, 0.0, 0.0, 0, 0};
    if (lane == 0) prev = zero;
    OctScan off = zero;
    total = zero;
    for (int k = 0; k < kTile / 64; k++) {
        if (k < w) off = oct_add(off, wsum[k]);
        total = oct_add(total, wsum[k]);
    }
    __syncthreads();   // (wsum is reused by the next call)
    return oct_add(off, prev);
}

__device__ __forceinline__ OctScan oct_item(const float4 p, const int cnt)
{
    const double m = (double)p.w;
    return OctScan{m, m * (double)p.x, m * (double)p.y, m * (double)p.z, cnt, cnt > 0 ? 1 : 0};
}

// per body: the nodes that start at it, its record in key order; per scan block: the block's sums
__global__ __launch_bounds__(kTile) void k_oct_scan_reduce(const float4* __restrict__ posm, const u64* __restrict__ keys,
                                                           const unsigned* __restrict__ idx, const int n, float4* __restrict__ sb,
                                                           unsigned char* __restrict__ cnt, OctScan* __restrict__ block_sums,
                                                           int* __restrict__ counters)
{
    OctScan mine{0.0, 0.0, 0.0, 0.0, 0, 0};
    int deepest = 0;
    const int j0 = blockIdx.x * kOctScanBlock + threadIdx.x * kOctScanPerThread;
    for (int u = 0; u < kOctScanPerThread; u++) {
        const int j = j0 + u;
        if (j >= n) break;
        const float4 p = posm[idx[j]];
        sb[j] = p;
        const u64 k = keys[j];
        const int cl = j == 0 ? -1 : oct_common(keys[j - 1], k);
        int c = 0;
        if (cl < kOctLevels) {   // the first body of its level-21 cell: it starts the cell's leaf and every node above that starts here
            const int e = oct_range_end(keys, j, n, kOctLevels);
            const int cr = e == n ? -1 : oct_common(k, keys[e]);
            int leaf = 1 + (cl > cr ? cl : cr);
            if (leaf > kOctLevels) leaf = kOctLevels;
            c = leaf - cl;
            deepest = leaf > deepest ? leaf : deepest;
            if (e - j > 1) {   // a multi-body leaf stands in for the reference's EPS merge only if its bodies ARE within EPS (nbody.rs:249)
                float lo[3] = {p.x, p.y, p.z}, hi[3] = {p.x, p.y, p.z};
                for (int t = j + 1; t < e; t++) {
                    const float4 q = posm[idx[t]];
                    lo[0] = fminf(lo[0], q.x); lo[1] = fminf(lo[1], q.y); lo[2] = fminf(lo[2], q.z);
                    hi[0] = fmaxf(hi[0], q.x); hi[1] = fmaxf(hi[1], q.y); hi[2] = fmaxf(hi[2], q.z);
                }
                if (!(__fsub_rn(hi[0], lo[0]) < kEps && __fsub_rn(hi[1], lo[1]) < kEps && __fsub_rn(hi[2], lo[2]) < kEps))
                    atomicAdd(&counters[2], 1);
            }
        }
        cnt[j] = (unsigned char)c;
        mine = oct_add(mine, oct_item(p, c));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) deepest = max(deepest, __shfl_xor(deepest, off));
    if ((threadIdx.x & 63) == 0) atomicMax(&counters[3], deepest);
    OctScan total;
    (void)oct_block_exclusive(mine, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup: block_sums[0..nb) -> their exclusive prefixes, block_sums[nb] = the grand total; counters[0] / [1] = nodes / leaves
__global__ __launch_bounds__(kTile) void k_oct_scan_blocks(OctScan* __restrict__ block_sums, const int nb, int* __restrict__ counters)
{
    const int per = (nb + kTile - 1) / kTile;
    const int a = (int)threadIdx.x * per, b = a + per < nb ? a + per : nb;
    OctScan mine{0.0, 0.0, 0.0, 0.0, 0, 0};
    for (int k = a; k < b; k++) mine = oct_add(mine, block_sums[k]);
    OctScan total;
    OctScan run = oct_block_exclusive(mine, total);
    for (int k = a; k < b; k++) {
        const OctScan v = block_sums[k];
        block_sums[k] = run;
        run = oct_add(run, v);
    }
    if (threadIdx.x == 0) {
        block_sums[nb] = total;
        counters[0] = total.cnt;
        counters[1] = total.ent;
    }
}

__global__ __launch_bounds__(kTile) void k_oct_scan_write(const float4* __restrict__ sb, const unsigned char* __restrict__ cnt, const int n,
                                                          const OctScan* __restrict__ block_sums, double* __restrict__ pm,
                                                          double* __restrict__ pmx, double* __restrict__ pmy, double* __restrict__ pmz,
                                                          int* __restrict__ base, int* __restrict__ ent)
{
    OctScan item[kOctScanPerThread];
    OctScan mine{0.0, 0.0, 0.0, 0.0, 0, 0};
    const int j0 = blockIdx.x * kOctScanBlock + threadIdx.x * kOctScanPerThread;
#pragma unroll
    for (int u = 0; u < kOctScanPerThread; u++) {
        const int j = j0 + u;
        item[u] = j < n ? oct_item(sb[j], (int)cnt[j]) : OctScan{0.0, 0.0, 0.0, 0.0, 0, 0};
        mine = oct_add(mine, item[u]);
    }
    OctScan total;
    OctScan run = oct_add(block_sums[blockIdx.x], oct_block_exclusive(mine, total));
#pragma unroll
    for (int u = 0; u < kOctScanPerThread; u++) {
        const int j = j0 + u;
        if (j <= n) {   // (entry n = the totals: written by whoever holds the slot behind the last body)
            pm[j] = run.m; pmx[j] = run.mx; pmy[j] = run.my; pmz[j] = run.mz;
            base[j] = run.cnt;
            ent[j] = run.ent;
        }
        run = oct_add(run, item[u]);
    }
}

// ---- node records ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTile) void k_oct_emit(const float4* __restrict__ sb, const u64* __restrict__ keys, const int n,
                                                    const double* __restrict__ pm, const double* __restrict__ pmx,
                                                    const double* __restrict__ pmy, const double* __restrict__ pmz,
                                                    const int* __restrict__ base, const int* __restrict__ ent,
                                                    const unsigned char* __restrict__ cnt, const float* __restrict__ box,
                                                    const int n_nodes, OctNode* __restrict__ out)
{
    const int k = blockIdx.x * kTile + threadIdx.x;
    if (k >= n_nodes) return;
    // the body the node starts at: the last a with base[a] <= k (base[a + 1] > k then says that a starts nodes at all)
    int lo = 0, hi = n;   // base[lo] <= k < base[hi] (base[0] = 0, base[n] = n_nodes)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (base[mid] <= k) lo = mid; else hi = mid;
    }
    const int a = lo;
    const u64 key = keys[a];
    const int cl = a == 0 ? -1 : oct_common(keys[a - 1], key);
    const int above = k - base[a];                 // nodes starting at a above this one
    const int depth = cl + 1 + above;
    const bool interior = above < (int)cnt[a] - 1; // a's leaf is the last node that starts at a
    const int b = oct_range_end(keys, a, n, depth);
    OctNode nd;
    if (b - a == 1) {   // a single body: its own record, so that its self term is m * 0 / (0 + EPS) = 0 exactly
        const float4 p = sb[a];
        nd.px = p.x; nd.py = p.y; nd.pz = p.z; nd.m = p.w;
    } else {
        double m, mx, my, mz;
        if (b - a <= 8) {
            m = mx = my = mz = 0.0;
            for (int t = a; t < b; t++) {
                const float4 p = sb[t];
                const double w = (double)p.w;
                m += w; mx += w * (double)p.x; my += w * (double)p.y; mz += w * (double)p.z;
            }
        } else {
            m = pm[b] - pm[a]; mx = pmx[b] - pmx[a]; my = pmy[b] - pmy[a]; mz = pmz[b] - pmz[a];
        }
        nd.px = (float)(mx / m); nd.py = (float)(my / m); nd.pz = (float)(mz / m); nd.m = (float)m;
    }
    float x1 = box[0], x2 = box[3];   // the box's x-extent: the x half of the descent, replayed along the key's digits
    for (int l = 0; l < depth; l++) {
        const float cx = __fmul_rn(__fadd_rn(x1, x2), 0.5f);
        if ((key >> (3 * (kOctLevels - 1 - l))) & 1ull) x1 = cx; else x2 = cx;
    }
    nd.s = __fsub_rn(x2, x1);
    nd.skip = base[b];
    nd.interior = interior ? 1 : 0;
    nd.rank = interior ? k - ent[a] : 0;   // ent[a] leaves precede a's nodes in pre-order; a's own leaf comes behind its interior nodes
    out[k] = nd;
}

// ---- entry points ------------------------------------------------------------------------------------------------------------
hipError_t oct_build_scan(const float4* posm, int n, void* workspace, size_t sort_tmp_bytes, hipStream_t stream)
{
    if (n <= 0) return hipErrorInvalidValue;
    const OctWs k = oct_carve(workspace, n, sort_tmp_bytes);
    const int nb = (n + kTile - 1) / kTile;
    const int parts = nb < kOctParts ? nb : kOctParts;
    hipLaunchKernelGGL(k_oct_bbox, dim3(parts), dim3(kTile), 0, stream, posm, n, k.part, k.counters);
    hipLaunchKernelGGL(k_oct_keys, dim3(nb), dim3(kTile), 0, stream, posm, n, k.part, parts, k.box, k.keys0, k.idx0);
    size_t tmp = sort_tmp_bytes;
    const hipError_t e = rocprim::radix_sort_pairs(k.sort_tmp, tmp, k.keys0, k.keys1, k.idx0, k.idx1, (size_t)n, 0, 3 * kOctLevels, stream);
    if (e != hipSuccess) return e;
    const int sblocks = (n + kOctScanBlock - 1) / kOctScanBlock;
    hipLaunchKernelGGL(k_oct_scan_reduce, dim3(sblocks), dim3(kTile), 0, stream, posm, k.keys1, k.idx1, n, k.sb, k.cnt, k.block_sums,
                       k.counters);
    hipLaunchKernelGGL(k_oct_scan_blocks, dim3(1), dim3(kTile), 0, stream, k.block_sums, sblocks, k.counters);
    // (n + 1 entries: one more slot than bodies)
    hipLaunchKernelGGL(k_oct_scan_write, dim3((n + 1 + kOctScanBlock - 1) / kOctScanBlock), dim3(kTile), 0, stream, k.sb, k.cnt, n,
                       k.block_sums, k.pm, k.pmx, k.pmy, k.pmz, k.base, k.ent);
    return hipGetLastError();
}

hipError_t oct_build_emit(int n, void* workspace, size_t sort_tmp_bytes, int n_nodes, OctNode* nodes, hipStream_t stream)
{
    if (n <= 0 || n_nodes <= 0) return hipErrorInvalidValue;
    const OctWs k = oct_carve(workspace, n, sort_tmp_bytes);
    hipLaunchKernelGGL(k_oct_emit, dim3((n_nodes + kTile - 1) / kTile), dim3(kTile), 0, stream, k.sb, k.keys1, n, k.pm, k.pmx, k.pmy, k.pmz,
                       k.base, k.ent, k.cnt, k.box, n_nodes, nodes);
    return hipGetLastError();
}

}  // namespace nbx
