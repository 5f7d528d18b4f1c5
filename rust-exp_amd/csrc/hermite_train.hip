// hermite_train.hip -- K10: Hermite block steps for SMALL blocks (at most kTrainMaxBlock = 64 due bodies), enqueued in trains,
// behind NBX_OPT_HERMITE_BLOCK_TRAIN.  K9 (hermite_block.hip) pays eight launches, one host read and a 56 us latency chain per
// block step whatever the block's size; almost every block of an adaptive run holds a handful of bodies.  Here a block step -- a
// "car" -- is TWO launches that take (t_next, n_active) and the list from device memory, so the host enqueues L cars per read:
//
//   k_train_sweep<DIM, PREDICT>   G workgroups of 256 threads; workgroup g owns the whole source tiles [tiles g / G, tiles (g + 1) / G)
//                                 (the range formula of the other sweeps).
//                                   targets   the first n_active threads predict the listed bodies to t_next (block_predict_body,
//                                             hermite_block_math.h) into LDS: 64 HermiteSrc records, 2 KB, zero past n_active
//                                   sources   SPLIT ACROSS LANES: lane tid takes j0 + tid, j0 + tid + 256, .. of the workgroup's range,
//                                             loads posm / vel / kept / bt of the body with coalesced vector loads and predicts it in
//                                             registers with the same function (so a target and its copy among the sources agree in
//                                             every bit and the self pair adds exact zeros); j >= n is the zero record.  There is no
//                                             source array, no scalar feeding and no dependent chain: at 65 536 bodies and 256 CUs a lane
//                                             evaluates ONE source
//                                   pairs     K8's arithmetic (hermite.hip): 24 VALU + v_rcp_f32 per pair at DIM = 3, 17 + 1 at DIM = 2; the
//                                             target's record is an LDS broadcast (two ds_read_b128, every lane the same address)
//                                   sums      targets are taken kChunk = 8 at a time: 48 accumulators per lane (the lane's sources are
//                                             predicted again per chunk: blocks of up to 8 bodies, the common ones, predict once).
//                                             THE ORDER, fixed by (n_pad, G) and the lane index only -- never by n_active, the slot or
//                                             the other bodies of the block:
//                                               1. per lane: its sources in ascending j, one FMA chain per sum
//                                               2. across the 64 lanes of a wave: a butterfly over lane distances 32, 16, 8, 4, 2, 1,
//                                                  each step adding the sums of lanes L and L ^ d (addition commutes, so both get the same
//                                                  bits).  The first four steps are HALVING: a lane hands over the half of its values its
//                                                  partner keeps (24, 12, 6, 3 exchanges instead of 48 each; 51 exchanges per chunk in
//                                                  all); which half is a matter of where the result lands, not of what is added to what.
//                                                  Lanes with lane % 4 == 0 end with sums 3 (lane / 4) .. + 2 of the chunk's 48
//                                               3. across the four waves: through LDS (red[4][384], 6 KB), ONE barrier after the last chunk,
//                                                  added in wave order 0, 1, 2, 3
//                                             partial[g][slot], 64 slots per workgroup.
//                                 PREDICT = false serves nbx_acc_jerk_subset: the bodies as they are, kept / bt not read, the count an
//                                 argument.  PREDICT = true returns at once, uniformly over the grid, when the pending block is larger
//                                 than 64 bodies or the train is marked finished: such a car is a no-op
//   k_train_finish                ONE workgroup of 1 024 threads (same no-op rule).
//                                   sum       16 threads per slot: thread (slot, part) adds the partials g in [G part / 16, G (part + 1) / 16)
//                                             in ascending g starting from zero, then the 16 parts meet in a butterfly over distances
//                                             8, 4, 2, 1.  Fixed by G alone
//                                   correct   block_correct_body (hermite_block_math.h: k_block_correct's corrector and level rule),
//                                             scattered to posm / vel / kept / bt.  t_next = 2^20 stores t = 0 and marks the train
//                                             finished: the macro-step is complete
//                                   schedule  after the barrier the same workgroup finds the next block over all n bodies: the minimum of
//                                             t_i + step_i (wave butterflies, 16 minima through LDS); then wave w owns the bodies
//                                             [w seg, (w + 1) seg), seg a multiple of 64: it counts its due bodies (ballots), the counts of
//                                             the waves below give its offset, and it writes its due indices in ascending order (ballot
//                                             ranks and a running offset over 64-body chunks taken in ascending order) -- the list
//                                             k_block_select_write would write.  Three passes over bt (8 bytes per body), no barrier inside
//                                             a pass.  HermiteHead {t_next, n_active} is written in place, so that K9's kernels can pick
//                                             up a large block from it; the train's own record (HermiteTrain: t_done, the block steps
//                                             run, their evaluations, the finished flag) lives in a buffer of its own
//   k_train_reset                 clears the train record at the start of a macro-step
// No atomics, no cooperative launch, no workgroup that waits on another: order comes from the stream alone.  No scratch.
#include <algorithm>

#include "hermite_block_math.h"

namespace nbx {

namespace {

constexpr int kChunk = 8;               // targets whose sums a lane holds at once
constexpr int kSums = 6 * kChunk;       // ... 48 accumulators
constexpr int kFinishThreads = 1024;
constexpr int kParts = 16;              // threads per slot in k_train_finish's sum

template <bool PREDICT>
__device__ __forceinline__ HermiteSrc train_record(const float4* __restrict__ posm, const float4* __restrict__ vel,
                                                   const HermiteAJ* __restrict__ kept, const HermiteBody* __restrict__ bt, const int i,
                                                   const int t_next, const HermiteLevels& lv)
{
    const float4 p = posm[i];
    const float4 v = vel[i];
    if (PREDICT) return block_predict_body(p, v, kept[i], bt[i], t_next, lv);
    return HermiteSrc{p.x, p.y, p.z, p.w, v.x, v.y, v.z, 0.f};
}

template <int DIM, bool PREDICT>
__global__ __launch_bounds__(kTile) void k_train_sweep(const float4* __restrict__ posm, const float4* __restrict__ vel,
                                                       const HermiteAJ* __restrict__ kept, const HermiteBody* __restrict__ bt, const int n,
                                                       const int tiles_total, const HermiteHead* __restrict__ head,
                                                       const HermiteTrain* __restrict__ train, const int* __restrict__ list, const int count,
                                                       const HermiteLevels lv, HermiteAJ* __restrict__ partial)
{
    __shared__ HermiteSrc tgt[kTrainMaxBlock];
    __shared__ float red[4][6 * kTrainMaxBlock];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    int t_next = 0, n_active = count;
    if (PREDICT) {
        t_next = head->t_next;
        n_active = head->n_active;
        if (train->finished) return;
    }
    if (n_active < 1 || n_active > kTrainMaxBlock) return;   // (uniform: a large block is K9's)

    if (tid < kTrainMaxBlock) {
        HermiteSrc r{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (tid < n_active) r = train_record<PREDICT>(posm, vel, kept, bt, list[tid], t_next, lv);
        tgt[tid] = r;
    }
    __syncthreads();

    const int split = (int)blockIdx.x, jsplit = (int)gridDim.x;
    const int j0 = (int)(((unsigned)tiles_total * (unsigned)split) / (unsigned)jsplit) * kTile;
    const int j1 = (int)(((unsigned)tiles_total * (unsigned)(split + 1)) / (unsigned)jsplit) * kTile;
    const int chunks = (n_active + kChunk - 1) / kChunk;
    for (int c = 0; c < chunks; c++) {
        float acc[kSums];
#pragma unroll
        for (int k = 0; k < kSums; k++) acc[k] = 0.f;
        for (int j = j0 + tid; j < j1; j += kTile) {
            HermiteSrc s{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (j < n) s = train_record<PREDICT>(posm, vel, kept, bt, j, t_next, lv);
#pragma unroll
            for (int k = 0; k < kChunk; k++) {
                const float4* rec = reinterpret_cast<const float4*>(&tgt[c * kChunk + k]);
                const float4 tp = rec[0], tv = rec[1];   // (x, y, z, m), (vx, vy, vz, 0): broadcasts
                const float dx = s.x - tp.x, dy = s.y - tp.y;
                const float wx = s.vx - tv.x, wy = s.vy - tv.y;
                float r2 = __builtin_fmaf(dx, dx, kEps);
                r2 = __builtin_fmaf(dy, dy, r2);
                float dw = dx * wx;
                dw = __builtin_fmaf(dy, wy, dw);
                float dz = 0.f, wz = 0.f;
                if (DIM == 3) {
                    dz = s.z - tp.z;
                    wz = s.vz - tv.z;
                    r2 = __builtin_fmaf(dz, dz, r2);
                    dw = __builtin_fmaf(dz, wz, dw);
                }
                const float inv = __builtin_amdgcn_rcpf(r2);
                const float mi = s.m * inv;
                const float beta = dw * (inv * -2.0f);
                acc[6 * k + 0] = __builtin_fmaf(mi, dx, acc[6 * k + 0]);
                acc[6 * k + 1] = __builtin_fmaf(mi, dy, acc[6 * k + 1]);
                acc[6 * k + 3] = __builtin_fmaf(mi, __builtin_fmaf(beta, dx, wx), acc[6 * k + 3]);
                acc[6 * k + 4] = __builtin_fmaf(mi, __builtin_fmaf(beta, dy, wy), acc[6 * k + 4]);
                if (DIM == 3) {
                    acc[6 * k + 2] = __builtin_fmaf(mi, dz, acc[6 * k + 2]);
                    acc[6 * k + 5] = __builtin_fmaf(mi, __builtin_fmaf(beta, dz, wz), acc[6 * k + 5]);
                }
            }
        }
        // the halving steps: a lane whose bit d is set keeps the upper half of its values and hands over the lower one
#pragma unroll
        for (int d = 32, half = kSums / 2; d >= 4; d >>= 1, half >>= 1) {
            const bool upper = (lane & d) != 0;
#pragma unroll
            for (int k = 0; k < half; k++) {
                const float mine = upper ? acc[k + half] : acc[k];
                const float theirs = __shfl_xor(upper ? acc[k] : acc[k + half], d);
                acc[k] = mine + theirs;
            }
        }
#pragma unroll
        for (int d = 2; d >= 1; d >>= 1) {
#pragma unroll
            for (int k = 0; k < 3; k++) acc[k] += __shfl_xor(acc[k], d);
        }
        if ((lane & 3) == 0) {   // sums 3 (lane / 4) .. + 2 of the chunk: (ax, ay, az) or (jx, jy, jz) of target lane / 8
            float* out = &red[wave][c * kSums + 3 * (lane >> 2)];
            out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2];
        }
    }
    __syncthreads();
    if (tid < n_active) {
        float q[6];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            q[k] = red[0][6 * tid + k];
#pragma unroll
            for (int w = 1; w < 4; w++) q[k] += red[w][6 * tid + k];
        }
        partial[(size_t)split * kTrainMaxBlock + tid] = HermiteAJ{make_float4(q[0], q[1], q[2], 0.f), make_float4(q[3], q[4], q[5], 0.f)};
    }
}

__device__ __forceinline__ bool due_at(const HermiteBody* bt, const int i, const int end, const int t_next)
{
    if (i >= end) return false;
    const HermiteBody b = bt[i];
    return b.t + step_of(b.level) == t_next;
}

__global__ __launch_bounds__(kFinishThreads) void k_train_finish(float4* __restrict__ posm, float4* __restrict__ vel,
                                                                 HermiteAJ* __restrict__ kept, HermiteBody* bt, const int n, int* list,
                                                                 HermiteHead* head, HermiteTrain* train,
                                                                 const HermiteAJ* __restrict__ partial, const int groups, const HermiteLevels lv)
{
    __shared__ int wave_min[kFinishThreads / 64];
    __shared__ int wave_count[kFinishThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t_next = head->t_next, n_active = head->n_active;
    if (train->finished || n_active < 1 || n_active > kTrainMaxBlock) return;

    // (a1, j1) of the block: 16 threads per slot, each a contiguous run of the G partials in ascending g
    const int slot = tid / kParts, part = tid % kParts;
    float q[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (slot < n_active) {
        const int g1 = (int)(((unsigned)groups * (unsigned)(part + 1)) / (unsigned)kParts);
        for (int g = (int)(((unsigned)groups * (unsigned)part) / (unsigned)kParts); g < g1; g++) {
            const HermiteAJ r = partial[(size_t)g * kTrainMaxBlock + slot];
            q[0] += r.a.x; q[1] += r.a.y; q[2] += r.a.z;
            q[3] += r.j.x; q[4] += r.j.y; q[5] += r.j.z;
        }
    }
#pragma unroll
    for (int d = kParts / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 6; k++) q[k] += __shfl_xor(q[k], d);
    }
    if (slot < n_active && part == 0)
        block_correct_body(posm, vel, kept, bt, list[slot], HermiteAJ{make_float4(q[0], q[1], q[2], 0.f), make_float4(q[3], q[4], q[5], 0.f)},
                           t_next, lv);
    __threadfence_block();
    __syncthreads();   // (the corrected bodies' (t, level) are what the scheduler below reads; the list is free to be rewritten)

    if (t_next == kHermiteTicks) {   // the macro-step is complete: every body stands at t = 0
        if (tid == 0) {
            train->t_done = t_next;
            train->steps += 1;
            train->evals += n_active;
            train->finished = 1;
        }
        return;
    }

    int r = 2 * kHermiteTicks;   // (above every time a body can be due at)
    for (int i = tid; i < n; i += kFinishThreads) {
        const HermiteBody b = bt[i];
        r = min(r, b.t + step_of(b.level));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) r = min(r, __shfl_xor(r, d));
    if (lane == 0) wave_min[wave] = r;
    __syncthreads();
    int t_new = wave_min[0];
#pragma unroll
    for (int w = 1; w < kFinishThreads / 64; w++) t_new = min(t_new, wave_min[w]);

    const int seg = ((n + kFinishThreads - 1) / kFinishThreads) * 64;   // bodies per wave: whole 64-body chunks
    const int lo = min(wave * seg, n), hi = min(lo + seg, n);
    int mine = 0;
    for (int base = lo; base < hi; base += 64) mine += __popcll(__ballot(due_at(bt, base + lane, hi, t_new)));
    if (lane == 0) wave_count[wave] = mine;
    __syncthreads();
    int offset = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kFinishThreads / 64; w++) {
        offset += w < wave ? wave_count[w] : 0;
        total += wave_count[w];
    }
    for (int base = lo; base < hi; base += 64) {
        const bool due = due_at(bt, base + lane, hi, t_new);
        const unsigned long long mask = __ballot(due);
        if (due) list[offset + __popcll(mask & ((1ull << lane) - 1ull))] = base + lane;   // (< the number of due bodies <= n)
        offset += __popcll(mask);
    }
    if (tid == 0) {
        head->t_next = t_new;
        head->n_active = total;
        train->t_done = t_next;
        train->steps += 1;
        train->evals += n_active;
    }
}

__global__ void k_train_reset(HermiteTrain* train)
{
    if (threadIdx.x == 0) *train = HermiteTrain{0, 0, 0, 0, 0};
}

}  // namespace

int hermite_train_groups(int tiles_total, int cu_count, int jsplit)
{
    const int g = jsplit > 0 ? jsplit : (cu_count > 0 ? cu_count : 256);
    return std::max(1, std::min(g, tiles_total));
}

hipError_t launch_train_reset(HermiteTrain* train, hipStream_t stream)
{
    hipLaunchKernelGGL(k_train_reset, dim3(1), dim3(64), 0, stream, train);
    return hipGetLastError();
}

hipError_t launch_train_sweep(const float4* posm, const float4* vel, const HermiteAJ* kept, const HermiteBody* bt, int n, int tiles_total,
                              int groups, int dim, const HermiteHead* head, const HermiteTrain* train, const int* list, int count,
                              const HermiteLevels& lv, HermiteAJ* partial, hipStream_t stream, ForceLaunch* info)
{
    if (n <= 0 || tiles_total <= 0) return hipSuccess;
    const bool predict = head != nullptr;
    if (groups < 1 || groups > tiles_total) return hipErrorInvalidValue;
    if (predict ? !(train && kept && bt) : (count < 1 || count > kTrainMaxBlock)) return hipErrorInvalidValue;
    if (info) *info = ForceLaunch{groups, kTile, groups, 1, dim, 42};
#define NBX_TRAIN_SWEEP(D, P) \
    hipLaunchKernelGGL((k_train_sweep<D, P>), dim3(groups), dim3(kTile), 0, stream, posm, vel, kept, bt, n, tiles_total, head, train, list, \
                       count, lv, partial)
    if (dim == 3) { if (predict) NBX_TRAIN_SWEEP(3, true); else NBX_TRAIN_SWEEP(3, false); }
    else          { if (predict) NBX_TRAIN_SWEEP(2, true); else NBX_TRAIN_SWEEP(2, false); }
#undef NBX_TRAIN_SWEEP
    return hipGetLastError();
}

hipError_t launch_train_finish(float4* posm, float4* vel, HermiteAJ* kept, HermiteBody* bt, int n, int* list, HermiteHead* head,
                               HermiteTrain* train, const HermiteAJ* partial, int groups, const HermiteLevels& lv, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_train_finish, dim3(1), dim3(kFinishThreads), 0, stream, posm, vel, kept, bt, n, list, head, train, partial, groups,
                       lv);
    return hipGetLastError();
}

}  // namespace nbx
