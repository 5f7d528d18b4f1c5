// hermite_block.hip -- K9: individual, hierarchical ("block") time steps for the 4th-order Hermite scheme of K8 (hermite.hip),
// behind nbx_step_hermite_block / nbx_acc_jerk_subset.
//
// Every body has its own step dt_max 2^-level, level 0 .. 20.  TIME IS INTEGER: a macro-step of dt_max is 2^20 ticks, a body at
// level l steps 2^(20 - l) of them, and "body i is due at t_next" is the exact compare t_i + step_i == t_next.  One block step:
//   k_block_next / _last       t_next = min_i (t_i + step_i): a fixed-order LDS tree per workgroup, then ONE workgroup over the
//                              partials (the pattern of k_hermite_dtmin)
//   k_block_select_count /     the due bodies' indices in ascending order into a compact list: count per workgroup (ballots),
//   k_block_select_write       the workgroups below summed, then rank inside the workgroup.  No atomics: the list is the same every
//                              time.  The last workgroup writes n_active beside t_next -- the 8 bytes the host reads to size the
//                              grids of what follows
//   k_block_predict            one 32-byte HermiteSrc record per body, predicted over ITS span t_next - t_i with k_hermite_predict's
//                              formula in its order.  A span that is the body's own step (every due body) takes the host-rounded
//                              (dt, c2, c3) of its level from the table; any other span dt = float(span) tick, c2 = (0.5 dt) dt,
//                              c3 = (c2 dt) (1/3), each product rounded on its own
//   k_block_sweep<DIM, T>      the hot kernel: (a, j) of the LISTED targets against all n_pad records.  The loop is k_hermite_sweep's,
//                              instruction for instruction: sources as SGPR operands through one wave-uniform 32-byte load, no LDS
//                              and no barrier inside; four waves hold the same 64 T targets and split the workgroup's source tiles;
//                              their sums meet in LDS once, in wave order.  What differs: lane k of a block GATHERS src[list[slot]]
//                              (two float4; idle lanes repeat the last listed target and write nothing); T = 1 or 2 is a template
//                              parameter, so that a block of 70 bodies does not occupy 128-target workgroups; and the source split S
//                              is sized by n_active (hermite_block_split), so that one target block still occupies the machine.
//                              Per target the order of summation is k_hermite_sweep's for the same S -- each wave its quarter in
//                              ascending j, waves in wave order, partials in ascending order -- whatever the target's slot: there is
//                              no lane-level source split.  partial[S][stride(n_active)], indexed by list slot
//   k_block_correct            one thread per list slot: the S partials in ascending order, the corrector of k_hermite_correct
//                              (hermite_math.h) with the level's h = dt / 2 and c12, scattered to posm / vel / kept of the body;
//                              t_i = t_next; then, unless levels are frozen, the new level from dt_req = eta |a1| / |j1| (the ratio of
//                              k_hermite_dtmin; |j1| = 0: no constraint): deeper while dt(level) > dt_req, else one level up if
//                              2 dt(level) <= dt_req and t_next is a multiple of the doubled step -- at most one doubling per update.
//                              The full Aarseth criterion needs a(2), a(3) from the differences a0 - a1, j0 - j1, which cancel in
//                              fp32: it is deliberately not used
//   k_block_init_levels        level = the first with dt(level) <= eta |a| / |j| of the kept pair, clamped to 0 .. 20; t_i = 0
//   k_block_keep               the partials of a slot in ascending order, (a, j) only (nbx_acc_jerk_subset)
// The prediction of a body and the corrector with its level rule live in hermite_block_math.h: K10 (hermite_train.hip) performs them too.
// All steps divide 2^20, so a macro-step ends with a block in which every body is due; that block's corrector leaves t_i = 0.
// Deterministic: no atomics anywhere, every order fixed by (n, the levels, S).
#include <algorithm>
#include <cmath>

#include "hermite_block_math.h"

namespace nbx {

namespace {

// Blocks below this many bodies run T = 1 (64-target workgroups).  Measured (docs/rounds/r10.md): T = 1 wins at every partial block
// size tried, 1 .. 65 536 of 262 144 bodies -- by 20 % where one workgroup row is all there is, by 3 - 6 % above; larger partial
// blocks were not measured and keep K8's T = 2, as the all-active block does by definition
constexpr int kTwoTargetsFrom = 131072;

__device__ __forceinline__ int tree_min(int* red, const int tid, int r)
{
    red[tid] = r;
    __syncthreads();
    for (int half = kTile / 2; half > 0; half >>= 1) {
        if (tid < half) red[tid] = min(red[tid], red[tid + half]);
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ int tree_sum(int* red, const int tid, int r)
{
    red[tid] = r;
    __syncthreads();
    for (int half = kTile / 2; half > 0; half >>= 1) {
        if (tid < half) red[tid] += red[tid + half];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(kTile) void k_block_next(const HermiteBody* __restrict__ bt, const int n, int* __restrict__ block_min)
{
    __shared__ int red[kTile];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kTile + tid;
    int r = 2 * kHermiteTicks;   // (above every time a body can be due at)
    if (i < n) {
        const HermiteBody b = bt[i];
        r = b.t + step_of(b.level);
    }
    r = tree_min(red, tid, r);
    if (tid == 0) block_min[blockIdx.x] = r;
}

__global__ __launch_bounds__(kTile) void k_block_next_last(const int* __restrict__ block_min, const int blocks, HermiteHead* __restrict__ head)
{
    __shared__ int red[kTile];
    const int tid = threadIdx.x;
    int r = 2 * kHermiteTicks;
    for (int b = tid; b < blocks; b += kTile) r = min(r, block_min[b]);
    r = tree_min(red, tid, r);
    if (tid == 0) head->t_next = r;
}

__device__ __forceinline__ bool is_due(const HermiteBody* __restrict__ bt, const int i, const int n, const int t_next)
{
    if (i >= n) return false;
    const HermiteBody b = bt[i];
    return b.t + step_of(b.level) == t_next;
}

__global__ __launch_bounds__(kTile) void k_block_select_count(const HermiteBody* __restrict__ bt, const int n,
                                                              const HermiteHead* __restrict__ head, int* __restrict__ counts)
{
    __shared__ int red[kTile];
    const int tid = threadIdx.x;
    const int c = tree_sum(red, tid, is_due(bt, blockIdx.x * kTile + tid, n, head->t_next) ? 1 : 0);
    if (tid == 0) counts[blockIdx.x] = c;
}

__global__ __launch_bounds__(kTile) void k_block_select_write(const HermiteBody* __restrict__ bt, const int n, HermiteHead* __restrict__ head,
                                                              const int* __restrict__ counts, int* __restrict__ list)
{
    __shared__ int red[kTile];
    __shared__ int wave_count[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * kTile + tid;
    int below = 0;   // the due bodies of the workgroups before this one
    for (int b = tid; b < (int)blockIdx.x; b += kTile) below += counts[b];
    below = tree_sum(red, tid, below);
    const bool due = is_due(bt, i, n, head->t_next);
    const unsigned long long mask = __ballot(due);
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int slot = below + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) slot += wave_count[w];
    if (due) list[slot] = i;   // (slot < the number of due bodies <= n)
    if (blockIdx.x == gridDim.x - 1 && tid == 0) head->n_active = below + wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

__global__ __launch_bounds__(kTile) void k_block_predict(const float4* __restrict__ posm, const float4* __restrict__ vel,
                                                         const HermiteAJ* __restrict__ kept, const HermiteBody* __restrict__ bt,
                                                         const int n, const int n_pad, const int t_next, const HermiteLevels lv,
                                                         HermiteSrc* __restrict__ src)
{
    const int i = blockIdx.x * kTile + threadIdx.x;
    if (i >= n_pad) return;
    HermiteSrc r{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < n) {
        r = block_predict_body(posm[i], vel[i], kept[i], bt[i], t_next, lv);   // (hermite_block_math.h: K10 predicts with it too)
    }
    src[i] = r;
}

template <int DIM, int T>
__global__ __launch_bounds__(kTile) void k_block_sweep(const HermiteSrc* __restrict__ src, const int* __restrict__ list,
                                                       const int n_active, const int tiles_total, HermiteAJ* __restrict__ partial,
                                                       const int stride)
{
    constexpr int kBlock = 64 * T;   // targets per workgroup
    __shared__ float red[4][6][kBlock];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = (int)blockIdx.y, jsplit = (int)gridDim.y;
    const int t0 = (int)blockIdx.x * kBlock;
    // this workgroup's whole tiles of sources, then this wave's quarter of them (a multiple of 64): k_hermite_sweep's ranges
    const int j0 = (int)(((unsigned)tiles_total * (unsigned)split) / (unsigned)jsplit) * kTile;
    const int j1 = (int)(((unsigned)tiles_total * (unsigned)(split + 1)) / (unsigned)jsplit) * kTile;
    const int quarter = (j1 - j0) >> 2;
    const int ja = j0 + quarter * wave, jb = ja + quarter;

    float x[T], y[T], z[T], vx[T], vy[T], vz[T];
    float ax[T], ay[T], az[T], jx[T], jy[T], jz[T];
#pragma unroll
    for (int k = 0; k < T; k++) {
        int slot = t0 + k * 64 + lane;
        slot = slot < n_active ? slot : n_active - 1;   // (idle lanes repeat the last listed target; nothing of theirs is written)
        const float4* rec = reinterpret_cast<const float4*>(src + list[slot]);
        const float4 p = rec[0], v = rec[1];
        x[k] = p.x; y[k] = p.y; z[k] = p.z; vx[k] = v.x; vy[k] = v.y; vz[k] = v.z;
        ax[k] = ay[k] = az[k] = jx[k] = jy[k] = jz[k] = 0.f;
    }
    if (ja < jb) {
        HermiteSrc next = src[ja];
#pragma unroll 2
        for (int j = ja; j < jb; j++) {
            const HermiteSrc s = next;
            next = src[j + 1 < jb ? j + 1 : j];   // the next record is on its way while this one is evaluated
#pragma unroll
            for (int k = 0; k < T; k++) {
                const float dx = s.x - x[k], dy = s.y - y[k];
                const float wx = s.vx - vx[k], wy = s.vy - vy[k];
                float r2 = __builtin_fmaf(dx, dx, kEps);
                r2 = __builtin_fmaf(dy, dy, r2);
                float dw = dx * wx;
                dw = __builtin_fmaf(dy, wy, dw);
                float dz = 0.f, wz = 0.f;
                if (DIM == 3) {
                    dz = s.z - z[k];
                    wz = s.vz - vz[k];
                    r2 = __builtin_fmaf(dz, dz, r2);
                    dw = __builtin_fmaf(dz, wz, dw);
                }
                const float inv = __builtin_amdgcn_rcpf(r2);
                const float mi = s.m * inv;
                const float beta = dw * (inv * -2.0f);
                ax[k] = __builtin_fmaf(mi, dx, ax[k]);
                ay[k] = __builtin_fmaf(mi, dy, ay[k]);
                jx[k] = __builtin_fmaf(mi, __builtin_fmaf(beta, dx, wx), jx[k]);
                jy[k] = __builtin_fmaf(mi, __builtin_fmaf(beta, dy, wy), jy[k]);
                if (DIM == 3) {
                    az[k] = __builtin_fmaf(mi, dz, az[k]);
                    jz[k] = __builtin_fmaf(mi, __builtin_fmaf(beta, dz, wz), jz[k]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < T; k++) {   // slot k * 64 + lane of the block: conflict-free rows
        red[wave][0][k * 64 + lane] = ax[k]; red[wave][1][k * 64 + lane] = ay[k]; red[wave][2][k * 64 + lane] = az[k];
        red[wave][3][k * 64 + lane] = jx[k]; red[wave][4][k * 64 + lane] = jy[k]; red[wave][5][k * 64 + lane] = jz[k];
    }
    __syncthreads();
    const int slot = t0 + tid;
    if (tid < kBlock && slot < n_active) {
        float q[6];
#pragma unroll
        for (int c = 0; c < 6; c++) {
            q[c] = red[0][c][tid];
#pragma unroll
            for (int w = 1; w < 4; w++) q[c] += red[w][c][tid];
        }
        partial[(size_t)split * stride + slot] = HermiteAJ{make_float4(q[0], q[1], q[2], 0.f), make_float4(q[3], q[4], q[5], 0.f)};
    }
}

__device__ __forceinline__ HermiteAJ sum_partials(const HermiteAJ* __restrict__ partial, const int jsplit, const int stride,
                                                  const int slot)
{
    HermiteAJ r = partial[slot];
    for (int s = 1; s < jsplit; s++) {
        const HermiteAJ q = partial[(size_t)s * stride + slot];
        r.a.x += q.a.x; r.a.y += q.a.y; r.a.z += q.a.z;
        r.j.x += q.j.x; r.j.y += q.j.y; r.j.z += q.j.z;
    }
    return r;
}

__global__ __launch_bounds__(kTile) void k_block_correct(float4* __restrict__ posm, float4* __restrict__ vel, HermiteAJ* __restrict__ kept,
                                                         HermiteBody* __restrict__ bt, const int* __restrict__ list, const int n_active,
                                                         const HermiteAJ* __restrict__ partial, const int jsplit, const int stride,
                                                         const int t_next, const HermiteLevels lv)
{
    const int slot = blockIdx.x * kTile + threadIdx.x;
    if (slot >= n_active) return;
    const int i = list[slot];
    block_correct_body(posm, vel, kept, bt, i, sum_partials(partial, jsplit, stride, slot), t_next, lv);   // (hermite_block_math.h)
}

__global__ __launch_bounds__(kTile) void k_block_keep(const int n_active, const HermiteAJ* __restrict__ partial, const int jsplit,
                                                      const int stride, HermiteAJ* __restrict__ out)
{
    const int slot = blockIdx.x * kTile + threadIdx.x;
    if (slot >= n_active) return;
    out[slot] = sum_partials(partial, jsplit, stride, slot);
}

__global__ __launch_bounds__(kTile) void k_block_init_levels(const HermiteAJ* __restrict__ kept, const int n, const HermiteLevels lv,
                                                             HermiteBody* __restrict__ bt)
{
    const int i = blockIdx.x * kTile + threadIdx.x;
    if (i >= n) return;
    int level = 0;
    if (lv.eta > 0.f) {
        const float dt_req = __fmul_rn(lv.eta, hermite_ratio(kept[i]));
        while (lv.dt[level] > dt_req && level < kHermiteMaxLevel) level++;
    }
    bt[i] = HermiteBody{0, level};
}

inline int blocks_of(int n) { return (n + kTile - 1) / kTile; }

}  // namespace

HermiteLevels hermite_levels(float dt_max, float eta)
{
    HermiteLevels lv;
    for (int l = 0; l <= kHermiteMaxLevel; l++) {
        const float dt = (float)std::ldexp((double)dt_max, -l);   // (exact: a power of two times dt_max)
        lv.dt[l] = dt;
        lv.c2[l] = (float)(0.5 * (double)dt * (double)dt);
        lv.c3[l] = (float)((double)dt * (double)dt * (double)dt / 6.0);
        lv.h[l] = 0.5f * dt;
        lv.c12[l] = (float)((double)dt * (double)dt / 12.0);
    }
    lv.tick = (float)std::ldexp((double)dt_max, -kHermiteMaxLevel);
    lv.eta = eta;
    return lv;
}

int hermite_block_targets(int n_active, int n) { return n_active == n || n_active >= kTwoTargetsFrom ? 2 : 1; }

int hermite_block_stride(int n_active, int t) { return ((n_active + 64 * t - 1) / (64 * t)) * (64 * t); }

int hermite_block_split(int n_active, int n, int tiles_total, int cu_count, int t)
{
    if (n_active == n) return hermite_split(n, tiles_total, cu_count);   // the all-active block IS the shared step's sweep
    // hermite_split's target -- 64 workgroups per CU where targets are scarce, 32 otherwise -- without its stop at 64: one target
    // block against every source must still reach all CUs.  Every wave keeps a whole tile; the grid's y extent ends at 65 535
    const int blocks = hermite_block_stride(n_active, t) / (64 * t);
    const long long want = (long long)(cu_count > 0 ? cu_count : 256) * (n_active < 131072 ? 64 : 32);
    long long s = 1;
    while (blocks * s < want && s < 65536) s *= 2;
    const int cap = std::min(65535, tiles_total / 4 > 1 ? tiles_total / 4 : 1);
    return s < cap ? (int)s : cap;
}

size_t hermite_block_workspace(int n) { return 2 + 2 * (size_t)blocks_of(n); }

hipError_t launch_block_init_levels(const HermiteAJ* kept, int n, const HermiteLevels& lv, HermiteBody* bt, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_block_init_levels, dim3(blocks_of(n)), dim3(kTile), 0, stream, kept, n, lv, bt);
    return hipGetLastError();
}

hipError_t launch_block_schedule(const HermiteBody* bt, int n, int* workspace, int* list, hipStream_t stream)
{
    if (n <= 0) return hipErrorInvalidValue;
    const int blocks = blocks_of(n);
    HermiteHead* head = reinterpret_cast<HermiteHead*>(workspace);
    int* block_min = workspace + 2;
    int* counts = block_min + blocks;
    hipLaunchKernelGGL(k_block_next, dim3(blocks), dim3(kTile), 0, stream, bt, n, block_min);
    hipLaunchKernelGGL(k_block_next_last, dim3(1), dim3(kTile), 0, stream, block_min, blocks, head);
    hipLaunchKernelGGL(k_block_select_count, dim3(blocks), dim3(kTile), 0, stream, bt, n, head, counts);
    hipLaunchKernelGGL(k_block_select_write, dim3(blocks), dim3(kTile), 0, stream, bt, n, head, counts, list);
    return hipGetLastError();
}

hipError_t launch_block_predict(const float4* posm, const float4* vel, const HermiteAJ* kept, const HermiteBody* bt, int n, int n_pad,
                                int t_next, const HermiteLevels& lv, HermiteSrc* src, hipStream_t stream)
{
    if (n_pad <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_block_predict, dim3(blocks_of(n_pad)), dim3(kTile), 0, stream, posm, vel, kept, bt, n, n_pad, t_next, lv, src);
    return hipGetLastError();
}

hipError_t launch_block_sweep(const HermiteSrc* src, const int* list, int n_active, int tiles_total, int jsplit, int dim, int t,
                              HermiteAJ* partial, hipStream_t stream, ForceLaunch* info)
{
    if (n_active <= 0 || tiles_total <= 0) return hipSuccess;
    if (jsplit < 1 || jsplit > tiles_total || jsplit > 65535 || (t != 1 && t != 2)) return hipErrorInvalidValue;
    const int stride = hermite_block_stride(n_active, t);
    const dim3 grid((unsigned)(stride / (64 * t)), (unsigned)jsplit);
    if (info) *info = ForceLaunch{(int)(grid.x * grid.y), kTile, jsplit, t, dim, 41};
#define NBX_BLOCK_SWEEP(D, TT) \
    hipLaunchKernelGGL((k_block_sweep<D, TT>), grid, dim3(kTile), 0, stream, src, list, n_active, tiles_total, partial, stride)
    if (dim == 3) { if (t == 2) NBX_BLOCK_SWEEP(3, 2); else NBX_BLOCK_SWEEP(3, 1); }
    else          { if (t == 2) NBX_BLOCK_SWEEP(2, 2); else NBX_BLOCK_SWEEP(2, 1); }
#undef NBX_BLOCK_SWEEP
    return hipGetLastError();
}

hipError_t launch_block_correct(float4* posm, float4* vel, HermiteAJ* kept, HermiteBody* bt, const int* list, int n_active,
                                const HermiteAJ* partial, int jsplit, int stride, int t_next, const HermiteLevels& lv, hipStream_t stream)
{
    if (n_active <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_block_correct, dim3(blocks_of(n_active)), dim3(kTile), 0, stream, posm, vel, kept, bt, list, n_active, partial,
                       jsplit, stride, t_next, lv);
    return hipGetLastError();
}

hipError_t launch_block_keep(int n_active, const HermiteAJ* partial, int jsplit, int stride, HermiteAJ* out, hipStream_t stream)
{
    if (n_active <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_block_keep, dim3(blocks_of(n_active)), dim3(kTile), 0, stream, n_active, partial, jsplit, stride, out);
    return hipGetLastError();
}

}  // namespace nbx
