// diag64.hip -- K7: the fp64 all-pairs sweep behind nbx_forces_f64 / nbx_conserved (force, potential and the conserved sums of
// the 1/r law in double precision, on the device).  Not the fp32 sweep with the types changed: that one wins by packed math and
// v_rcp_f32, and fp64 has neither.  What carries over is the feeding (variant 6): sources come through the SCALAR cache.
//
//   k_widen64     posm[0..n) -> double4 (x, y, z, m), 32 B per body, once per call (exact).  A wave-uniform index into this
//                 array is one s_load_dwordx8, and the fp64 VALU instructions take the source components straight from SGPR
//                 pairs -- one scalar operand per instruction, the constant-bus limit -- so the loop has no v_cvt_f64_f32, no LDS
//                 and no barrier.  Only the true n records exist: the padding of posm is never swept (no logarithm of a pad).
//   k_sweep64     a workgroup = 4 wave64 that hold the SAME 64 * T targets, T per lane in fp64 registers (x, y, z, fx, fy, fz and,
//                 with POT, phi), and split the workgroup's source range four ways; every scalar source load serves T pair
//                 evaluations and T independent reciprocal chains cover each other's latency.  The four waves' sums meet in
//                 LDS once, added in wave order.  Grid = (target blocks, S): S source ranges, so that a small system still fills
//                 the CUs; partial[S][stride] double4.
//                 Per pair and target: 3 subtractions, 3 FMAs for r2 = |d|^2 + eps, v_rcp_f64 + two Newton steps (4 FMAs: the
//                 seed is good to ~2^-26, two steps leave ~1 ulp; r2 >= eps is always a normal number), m_j * inv, 3 FMAs: 14 fp64
//                 VALU instructions + 1 v_rcp_f64 = 25 flop as the kernel executes them (FMA = 2).  POT adds m_j * log(r2) with the
//                 device library's fp64 log (<= 1 ulp); the 1/2 is applied once, by k_reduce64.
//                 The pair j = i: its force term is an exact zero (d = 0), its potential term m_i ln(eps) is not -- adding it
//                 and taking it out again would cost a rounding of |m_i ln(eps)|, more than a sum of small terms allows -- so
//                 the part of a wave's source range that meets the workgroup's own targets (at most 64 * T sources of the whole
//                 sweep) runs a loop that predicates the potential on the index; every other source runs the plain loop.
//   k_newton64    the same sweep for the Newtonian law (NBX_OPT_LAW = 1; described where it stands).
//   k_reduce64    per target: the S partials in ascending order, force times m_i, potential times 1/2 (times 1 under the Newtonian
//                 law) -> double4 (Fx, Fy, Fz, phi).
//   k_conserved64 the 12 sums of nbx_conserved_id: one body per thread, a fixed-order LDS tree per workgroup, then ONE workgroup
//                 over the partials in index order.  Every product of two widened floats is exact in fp64.
// Everything is deterministic: no atomics, every order fixed by the launch shape, which depends on (n, slab, CU count) only.
#include "kernels.h"

namespace nbx {

namespace {

constexpr int kT = kSweep64Targets;
static_assert(kT == 1 || kT == 2 || kT == 4, "targets per lane: 1, 2 or 4");
constexpr double kEps64 = (double)kEps;

__global__ __launch_bounds__(kTile) void k_widen64(const float4* __restrict__ posm, double4* __restrict__ src64, const int n)
{
    const int i = blockIdx.x * kTile + threadIdx.x;
    if (i >= n) return;
    const float4 p = posm[i];
    src64[i] = make_double4((double)p.x, (double)p.y, (double)p.z, (double)p.w);
}

struct Targets64 {
    double x[kT], y[kT], z[kT], fx[kT], fy[kT], fz[kT], ph[kT];
    int self[kT];   // global body index (SELF loops only)
};

// sources [ja, jb) against the lane's T targets.  j is wave-uniform: src64[j] is a scalar load.
template <bool POT, bool SELF>
__device__ __forceinline__ void sweep_range(const double4* __restrict__ src64, const int ja, const int jb, Targets64& t)
{
    if (ja >= jb) return;
    double4 next = src64[ja];
#pragma unroll 2
    for (int j = ja; j < jb; j++) {
        const double4 s = next;
        next = src64[j + 1 < jb ? j + 1 : j];   // the next record is on its way while this one is evaluated
#pragma unroll
        for (int k = 0; k < kT; k++) {
            const double dx = s.x - t.x[k];
            const double dy = s.y - t.y[k];
            const double dz = s.z - t.z[k];
            double r2 = __builtin_fma(dx, dx, kEps64);
            r2 = __builtin_fma(dy, dy, r2);
            r2 = __builtin_fma(dz, dz, r2);
            double inv = __builtin_amdgcn_rcp(r2);
            double err = __builtin_fma(-r2, inv, 1.0);
            inv = __builtin_fma(inv, err, inv);
            err = __builtin_fma(-r2, inv, 1.0);
            inv = __builtin_fma(inv, err, inv);
            const double sc = s.w * inv;
            t.fx[k] = __builtin_fma(sc, dx, t.fx[k]);
            t.fy[k] = __builtin_fma(sc, dy, t.fy[k]);
            t.fz[k] = __builtin_fma(sc, dz, t.fz[k]);
            if (POT) {
                double u = s.w * log(r2);
                if (SELF) u = j == t.self[k] ? 0.0 : u;
                t.ph[k] += u;
            }
        }
    }
}

template <bool POT>
__global__ __launch_bounds__(kTile) void k_sweep64(const float4* __restrict__ posm, const double4* __restrict__ src64, const int lo,
                                                   const int n_targets, const int n_sources, const int stride,
                                                   double4* __restrict__ partial)
{
    constexpr int kBlock = 64 * kT;          // targets per workgroup
    constexpr int kAcc = POT ? 4 : 3;
    __shared__ double red[4][kAcc][kBlock];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = blockIdx.x * kBlock;
    // this workgroup's source range, then this wave's quarter of it
    // (the first n % S ranges and the first len % 4 quarters are one source longer)
    const int base = n_sources / (int)gridDim.y, rem = n_sources % (int)gridDim.y, sy = (int)blockIdx.y;
    const int j0 = sy * base + (sy < rem ? sy : rem), len = base + (sy < rem ? 1 : 0);
    const int ja = j0 + (len >> 2) * wave + (wave < (len & 3) ? wave : (len & 3));
    const int jb = ja + (len >> 2) + (wave < (len & 3) ? 1 : 0);
    Targets64 t;
#pragma unroll
    for (int k = 0; k < kT; k++) {
        int it = t0 + k * 64 + lane;
        it = it < n_targets ? it : n_targets - 1;   // (idle lanes repeat the last target; nothing of theirs is written)
        const float4 p = posm[lo + it];
        t.x[k] = (double)p.x; t.y[k] = (double)p.y; t.z[k] = (double)p.z;
        t.fx[k] = t.fy[k] = t.fz[k] = t.ph[k] = 0.0;
        t.self[k] = lo + it;
    }
    if (POT) {
        // sources that are this workgroup's own targets: bodies [g0, g1)
        const int g0 = lo + t0, g1 = g0 + kBlock;
        int sa = ja > g0 ? ja : g0, sb = jb < g1 ? jb : g1;
        if (sa >= sb) sa = sb = jb;   // none: [ja, jb) and an empty range remain
        sweep_range<true, true>(src64, sa, sb, t);
#pragma unroll 1
        for (int part = 0; part < 2; part++) sweep_range<true, false>(src64, part ? sb : ja, part ? jb : sa, t);
    } else {
        sweep_range<false, false>(src64, ja, jb, t);
    }
#pragma unroll
    for (int k = 0; k < kT; k++) {   // target k * 64 + lane of the block: conflict-free rows
        red[wave][0][k * 64 + lane] = t.fx[k];
        red[wave][1][k * 64 + lane] = t.fy[k];
        red[wave][2][k * 64 + lane] = t.fz[k];
        if (POT) red[wave][kAcc - 1][k * 64 + lane] = t.ph[k];
    }
    __syncthreads();
    const int it = t0 + tid;
    if (tid < kBlock && it < n_targets) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < kAcc; q++) {
            a[q] = red[0][q][tid];
#pragma unroll
            for (int w = 1; w < 4; w++) a[q] += red[w][q][tid];
        }
        partial[(size_t)blockIdx.y * stride + it] = make_double4(a[0], a[1], a[2], a[3]);
    }
}

// K7's sibling for the Newtonian law (NBX_OPT_LAW = 1): F_i = m_i sum_j m_j d s^(-3/2), phi_i = -sum_{j != i} m_j s^(-1/2),
// s = |d|^2 + eps.  K7's design unchanged -- k_widen64 records, T targets per lane, four waves splitting the source range and
// meeting in LDS in wave order, sweep64_split / sweep64_stride, partial[S][stride] -- with another pair evaluation:
//   u = s^(-1/2): v_rsq_f64, then TWO Newton steps y <- y + (y/2)(1 - (s y) y), each a multiply, an FMA for the residual, a multiply
//   by 1/2 (exact) and an FMA.  A step squares the relative error (x 3/2): whatever the seed is good to beyond 2^-14, the second
//   step leaves less than 2^-53 of it.  What remains are the roundings of the last step: the product s y (it enters the residual
//   absolutely and u by half: 1/2) and the closing FMA (1) -- 3/2 roundings, charged as 2; s >= eps is always a normal number.
//   m_j u^3 = (m_j u)(u u): three multiplies, then the three accumulating FMAs; 17 fp64 VALU instructions + 1 v_rsq_f64.
//   POT: phi -= m_j u is ONE more FMA (K7 pays a library logarithm there).  The template is kept all the same: without the
//   potential the kernel needs neither the accumulator nor the own-targets loop (the always-accumulating form was not measured).
// The pair j = i: its force term is an exact zero, its potential term -m_i / sqrt(eps) is not and is predicated away by index in
// the same "own targets" sub-range loop K7 uses.  Coincident distinct bodies contribute the finite -m_j / sqrt(eps).
template <bool POT, bool SELF>
__device__ __forceinline__ void newton_range(const double4* __restrict__ src64, const int ja, const int jb, Targets64& t)
{
    if (ja >= jb) return;
    double4 next = src64[ja];
#pragma unroll 2
    for (int j = ja; j < jb; j++) {
        const double4 s = next;
        next = src64[j + 1 < jb ? j + 1 : j];   // the next record is on its way while this one is evaluated
#pragma unroll
        for (int k = 0; k < kT; k++) {
            const double dx = s.x - t.x[k];
            const double dy = s.y - t.y[k];
            const double dz = s.z - t.z[k];
            double r2 = __builtin_fma(dx, dx, kEps64);
            r2 = __builtin_fma(dy, dy, r2);
            r2 = __builtin_fma(dz, dz, r2);
            double u = __builtin_amdgcn_rsq(r2);
#pragma unroll
            for (int step = 0; step < 2; step++) {
                const double err = __builtin_fma(-(r2 * u), u, 1.0);
                u = __builtin_fma(0.5 * u, err, u);
            }
            const double mu = s.w * u;
            const double sc = mu * (u * u);
            t.fx[k] = __builtin_fma(sc, dx, t.fx[k]);
            t.fy[k] = __builtin_fma(sc, dy, t.fy[k]);
            t.fz[k] = __builtin_fma(sc, dz, t.fz[k]);
            if (POT) {
                double w = s.w;
                if (SELF) w = j == t.self[k] ? 0.0 : w;
                t.ph[k] = __builtin_fma(-w, u, t.ph[k]);
            }
        }
    }
}

template <bool POT>
__global__ __launch_bounds__(kTile) void k_newton64(const float4* __restrict__ posm, const double4* __restrict__ src64, const int lo,
                                                    const int n_targets, const int n_sources, const int stride,
                                                    double4* __restrict__ partial)
{
    constexpr int kBlock = 64 * kT;          // targets per workgroup
    constexpr int kAcc = POT ? 4 : 3;
    __shared__ double red[4][kAcc][kBlock];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = blockIdx.x * kBlock;
    // this workgroup's source range, then this wave's quarter of it, exactly as k_sweep64 cuts them
    const int base = n_sources / (int)gridDim.y, rem = n_sources % (int)gridDim.y, sy = (int)blockIdx.y;
    const int j0 = sy * base + (sy < rem ? sy : rem), len = base + (sy < rem ? 1 : 0);
    const int ja = j0 + (len >> 2) * wave + (wave < (len & 3) ? wave : (len & 3));
    const int jb = ja + (len >> 2) + (wave < (len & 3) ? 1 : 0);
    Targets64 t;
#pragma unroll
    for (int k = 0; k < kT; k++) {
        int it = t0 + k * 64 + lane;
        it = it < n_targets ? it : n_targets - 1;   // (idle lanes repeat the last target; nothing of theirs is written)
        const float4 p = posm[lo + it];
        t.x[k] = (double)p.x; t.y[k] = (double)p.y; t.z[k] = (double)p.z;
        t.fx[k] = t.fy[k] = t.fz[k] = t.ph[k] = 0.0;
        t.self[k] = lo + it;
    }
    if (POT) {
        const int g0 = lo + t0, g1 = g0 + kBlock;   // sources that are this workgroup's own targets: bodies [g0, g1)
        int sa = ja > g0 ? ja : g0, sb = jb < g1 ? jb : g1;
        if (sa >= sb) sa = sb = jb;   // none: [ja, jb) and an empty range remain
        newton_range<true, true>(src64, sa, sb, t);
#pragma unroll 1
        for (int part = 0; part < 2; part++) newton_range<true, false>(src64, part ? sb : ja, part ? jb : sa, t);
    } else {
        newton_range<false, false>(src64, ja, jb, t);
    }
#pragma unroll
    for (int k = 0; k < kT; k++) {   // target k * 64 + lane of the block: conflict-free rows
        red[wave][0][k * 64 + lane] = t.fx[k];
        red[wave][1][k * 64 + lane] = t.fy[k];
        red[wave][2][k * 64 + lane] = t.fz[k];
        if (POT) red[wave][kAcc - 1][k * 64 + lane] = t.ph[k];
    }
    __syncthreads();
    const int it = t0 + tid;
    if (tid < kBlock && it < n_targets) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < kAcc; q++) {
            a[q] = red[0][q][tid];
#pragma unroll
            for (int w = 1; w < 4; w++) a[q] += red[w][q][tid];
        }
        partial[(size_t)blockIdx.y * stride + it] = make_double4(a[0], a[1], a[2], a[3]);
    }
}

// w_scale: what the summed .w is multiplied by -- 1/2 for K7's sum of m_j ln(s), 1 for the Newtonian -sum m_j / sqrt(s)
__global__ __launch_bounds__(kTile) void k_reduce64(const float4* __restrict__ posm, const int lo, const int n_targets,
                                                    const double4* __restrict__ partial, const int split, const int stride,
                                                    double4* __restrict__ out, const double w_scale)
{
    const int i = blockIdx.x * kTile + threadIdx.x;
    if (i >= n_targets) return;
    double4 a = partial[i];
    for (int s = 1; s < split; s++) {
        const double4 q = partial[(size_t)s * stride + i];
        a.x += q.x; a.y += q.y; a.z += q.z; a.w += q.w;
    }
    const double m = (double)posm[lo + i].w;
    out[i] = make_double4(m * a.x, m * a.y, m * a.z, w_scale * a.w);
}

constexpr int kCons = 12;        // NBX_CONS_COUNT
constexpr int kConsChunks = 16;  // the last workgroup: 16 runs of partials per sum, then the 16 in order

__global__ __launch_bounds__(kTile) void k_conserved64(const float4* __restrict__ posm, const int lo, const int n_targets,
                                                       const float4* __restrict__ vel, const double4* __restrict__ out,
                                                       double* __restrict__ block_sums)
{
    __shared__ double red[kCons][kTile];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kTile + tid;
    double q[kCons];
#pragma unroll
    for (int k = 0; k < kCons; k++) q[k] = 0.0;
    if (i < n_targets) {
        const float4 p = posm[lo + i];
        const float4 u = vel[i];
        const double x = p.x, y = p.y, z = p.z, m = p.w, vx = u.x, vy = u.y, vz = u.z;
        q[0] = 0.5 * (m * (vx * vx + vy * vy + vz * vz));
        q[1] = 0.5 * (m * out[i].w);
        q[2] = m;
        q[3] = m * vx; q[4] = m * vy; q[5] = m * vz;
        q[6] = m * (y * vz - z * vy); q[7] = m * (z * vx - x * vz); q[8] = m * (x * vy - y * vx);
        q[9] = m * x; q[10] = m * y; q[11] = m * z;
    }
#pragma unroll
    for (int k = 0; k < kCons; k++) red[k][tid] = q[k];
    __syncthreads();
    for (int half = kTile / 2; half > 0; half >>= 1) {
        if (tid < half) {
#pragma unroll
            for (int k = 0; k < kCons; k++) red[k][tid] += red[k][tid + half];
        }
        __syncthreads();
    }
    if (tid < kCons) block_sums[(size_t)blockIdx.x * kCons + tid] = red[tid][0];
}

__global__ __launch_bounds__(kTile) void k_conserved64_last(const double* __restrict__ block_sums, const int blocks,
                                                            double* __restrict__ sums)
{
    __shared__ double red[kConsChunks][16];
    const int k = threadIdx.x & 15, chunk = threadIdx.x >> 4;   // 16 x 16 threads; sums 12 .. 15 idle
    const int per = (blocks + kConsChunks - 1) / kConsChunks;
    const int b0 = chunk * per, b1 = b0 + per < blocks ? b0 + per : blocks;
    double a = 0.0;
    if (k < kCons)
        for (int b = b0; b < b1; b++) a += block_sums[(size_t)b * kCons + k];
    red[chunk][k] = a;
    __syncthreads();
    if (threadIdx.x < kCons) {
        double total = red[0][threadIdx.x];
        for (int c = 1; c < kConsChunks; c++) total += red[c][threadIdx.x];
        sums[threadIdx.x] = total;
    }
}

}  // namespace

hipError_t launch_widen64(const float4* posm, double4* src64, int n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_widen64, dim3((n + kTile - 1) / kTile), dim3(kTile), 0, stream, posm, src64, n);
    return hipGetLastError();
}

int sweep64_stride(int n_targets)
{
    constexpr int block = 64 * kT;
    return ((n_targets + block - 1) / block) * block;
}

int sweep64_split(int n_targets, int n_sources, int cu_count)
{
    // <= 128 VGPRs: four waves per SIMD, i.e. four workgroups (one wave per SIMD each) resident per CU
    const int blocks = sweep64_stride(n_targets) / (64 * kT);
    const int want = 4 * (cu_count > 0 ? cu_count : 256);
    int s = blocks > 0 ? (want + blocks - 1) / blocks : 1;
    const int cap = n_sources / 64;
    s = s < cap ? s : cap;
    return s > 1 ? s : 1;
}

hipError_t launch_sweep64(const float4* posm, const double4* src64, int lo, int n_targets, int n_sources, int split, bool pot,
                          double4* partial, hipStream_t stream, ForceLaunch* info)
{
    if (n_targets <= 0 || n_sources <= 0) return hipSuccess;
    if (split < 1 || split > 65535) return hipErrorInvalidValue;
    const int stride = sweep64_stride(n_targets);
    const dim3 grid((unsigned)(stride / (64 * kT)), (unsigned)split);
    if (info) *info = ForceLaunch{(int)(grid.x * grid.y), kTile, split, kT, 3, 64};
    if (pot) hipLaunchKernelGGL(k_sweep64<true>, grid, dim3(kTile), 0, stream, posm, src64, lo, n_targets, n_sources, stride, partial);
    else     hipLaunchKernelGGL(k_sweep64<false>, grid, dim3(kTile), 0, stream, posm, src64, lo, n_targets, n_sources, stride, partial);
    return hipGetLastError();
}

hipError_t launch_newton64(const float4* posm, const double4* src64, int lo, int n_targets, int n_sources, int split, bool pot,
                           double4* partial, hipStream_t stream, ForceLaunch* info)
{
    if (n_targets <= 0 || n_sources <= 0) return hipSuccess;
    if (split < 1 || split > 65535) return hipErrorInvalidValue;
    const int stride = sweep64_stride(n_targets);
    const dim3 grid((unsigned)(stride / (64 * kT)), (unsigned)split);
    if (info) *info = ForceLaunch{(int)(grid.x * grid.y), kTile, split, kT, 3, 65};
    if (pot) hipLaunchKernelGGL(k_newton64<true>, grid, dim3(kTile), 0, stream, posm, src64, lo, n_targets, n_sources, stride, partial);
    else     hipLaunchKernelGGL(k_newton64<false>, grid, dim3(kTile), 0, stream, posm, src64, lo, n_targets, n_sources, stride, partial);
    return hipGetLastError();
}

hipError_t launch_reduce64(const float4* posm, int lo, int n_targets, const double4* partial, int split, double4* out,
                           hipStream_t stream, double w_scale)
{
    if (n_targets <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_reduce64, dim3((n_targets + kTile - 1) / kTile), dim3(kTile), 0, stream, posm, lo, n_targets, partial,
                       split, sweep64_stride(n_targets), out, w_scale);
    return hipGetLastError();
}

size_t conserved64_workspace(int n_targets) { return (size_t)((n_targets + kTile - 1) / kTile) * kCons; }

hipError_t launch_conserved64(const float4* posm, int lo, int n_targets, const float4* vel, const double4* out, double* workspace,
                              double* sums, hipStream_t stream)
{
    const int blocks = (n_targets + kTile - 1) / kTile;   // (0 bodies: the last kernel alone writes twelve zeros)
    if (blocks > 0)
        hipLaunchKernelGGL(k_conserved64, dim3(blocks), dim3(kTile), 0, stream, posm, lo, n_targets, vel, out, workspace);
    hipLaunchKernelGGL(k_conserved64_last, dim3(1), dim3(kTile), 0, stream, workspace, blocks, sums);
    return hipGetLastError();
}

}  // namespace nbx
