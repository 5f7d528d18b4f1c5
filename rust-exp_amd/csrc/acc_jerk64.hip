// acc_jerk64.hip -- K12: the fp64 acceleration + jerk sweep behind nbx_acc_jerk_f64, for both laws (NBX_OPT_LAW), over all bodies
// or a list of targets.  The arbiter of the quantity the Hermite family (K8 - K10) lives on:
//   law 0   a_i = sum_j m_j d / s,          j_i = sum_j m_j ( w / s - 2 (d.w) d / s^2 )
//   law 1   a_i = sum_j m_j d s^(-3/2),     j_i = sum_j m_j ( w s^(-3/2) - 3 (d.w) d s^(-5/2) )
// d = p_j - p_i, w = v_j - v_i, s = |d|^2 + eps, eps = (double)kEps; always 3-D (z = 0 gives the planar law exactly).
// The pair j = i is exact zeros under both laws (d = w = 0), distinct bodies at one position give zero acceleration and the finite
// jerk m_j w / eps (m_j w eps^(-3/2)): the loop has no index test, and no pad record exists to be swept.
//
//   k_widen_aj64    posm, vel -> one 64-byte record per body, (x, y, z, m, vx, vy, vz, 0) as doubles (exact), the true n only.  A
//                   wave-uniform index into this array is a 16-dword scalar load, and the fp64 VALU takes the components straight
//                   from SGPR pairs -- one scalar operand per instruction, the constant-bus limit, which is why every line of the
//                   pair arithmetic below has exactly one source component in it.  No v_cvt, no LDS and no barrier in the loop;
//                   the next record loads while the current one is evaluated.
//   k_acc_jerk64    <LAW, T>: a workgroup = 4 wave64 that hold the SAME 64 T targets, T per lane: position, velocity and six sums in
//                   fp64 = 24 VGPRs per target.  Targets are GATHERED: slot k 64 + lane of a block reads record list[slot], or
//                   record slot when there is no list; idle lanes repeat the last listed target and write nothing.  The four waves
//                   split the workgroup's source range four ways (K7's n-based cut: no tiles, no pads) and meet once: waves 1 - 3
//                   leave their sums in LDS, red[3][6][64 T] doubles (18 KB at T = 2, 36 KB at T = 4 -- four workgroups per CU
//                   fit the 160 KB at every T, which four rows would not at T = 4), and wave 0 adds them to its own registers in
//                   wave order.  Grid = (target blocks, S source ranges); partial[S][stride] of two double4.  The order of
//                   summation for a target is: ascending j inside a wave's quarter, the quarters in wave order, the S ranges
//                   ascending (k_reduce_aj64) -- a function of (n, S) alone, not of T, the slot, the list's length or its other
//                   bodies.  Every multiply-add is written as an explicit fma, so no T contracts differently from another.
//                   Per pair and target, law 0: 6 subtractions, 3 FMAs for s, 1 multiply + 2 FMAs for d.w, v_rcp_f64 + two Newton
//                   steps (4 FMAs, as K7), mi = m_j inv, -2 inv (exact), beta = (d.w)(-2 inv), 3 FMAs for u = w + beta d, 6
//                   accumulating FMAs: 28 fp64 VALU instructions + 1 v_rcp_f64 = 47 flop as executed (FMA = 2).
//                   Law 1: u = s^(-1/2) by v_rsq_f64 + two Newton steps as k_newton64 takes them (2 multiplies + 2 FMAs each: 8),
//                   u2 = u u, mi = (m_j u) u2, -3 u2, beta = (d.w)(-3 u2), the same tail: 34 fp64 VALU instructions + 1 v_rsq_f64 =
//                   54 flop.
//   k_reduce_aj64   per slot: the S partials in ascending order -> (a, j) of the slot.
// Everything is deterministic: no atomics, every order fixed by the launch shape.
#include "kernels.h"

namespace nbx {

namespace {

constexpr double kEps64 = (double)kEps;

__global__ __launch_bounds__(kTile) void k_widen_aj64(const float4* __restrict__ posm, const float4* __restrict__ vel,
                                                      AccJerk64Src* __restrict__ src, const int n)
{
    const int i = blockIdx.x * kTile + threadIdx.x;
    if (i >= n) return;
    const float4 p = posm[i], v = vel[i];
    double4* rec = reinterpret_cast<double4*>(src + i);
    rec[0] = make_double4((double)p.x, (double)p.y, (double)p.z, (double)p.w);
    rec[1] = make_double4((double)v.x, (double)v.y, (double)v.z, 0.0);
}

template <int T>
struct TargetsAJ64 {
    double x[T], y[T], z[T], vx[T], vy[T], vz[T];
    double ax[T], ay[T], az[T], jx[T], jy[T], jz[T];
};

// sources [ja, jb) against the lane's T targets.  j is wave-uniform: src[j] is a scalar load.
template <int LAW, int T>
__device__ __forceinline__ void sweep_aj64(const AccJerk64Src* __restrict__ src, const int ja, const int jb, TargetsAJ64<T>& t)
{
    if (ja >= jb) return;
    AccJerk64Src next = src[ja];
#pragma unroll 2
    for (int j = ja; j < jb; j++) {
        const AccJerk64Src s = next;
        next = src[j + 1 < jb ? j + 1 : j];   // the next record is on its way while this one is evaluated
#pragma unroll
        for (int k = 0; k < T; k++) {
            const double dx = s.x - t.x[k];
            const double dy = s.y - t.y[k];
            const double dz = s.z - t.z[k];
            const double wx = s.vx - t.vx[k];
            const double wy = s.vy - t.vy[k];
            const double wz = s.vz - t.vz[k];
            double r2 = __builtin_fma(dx, dx, kEps64);
            r2 = __builtin_fma(dy, dy, r2);
            r2 = __builtin_fma(dz, dz, r2);
            double dw = dx * wx;
            dw = __builtin_fma(dy, wy, dw);
            dw = __builtin_fma(dz, wz, dw);
            double mi, beta;
            if (LAW == 0) {
                double inv = __builtin_amdgcn_rcp(r2);   // r2 >= eps: always a normal number
                double err = __builtin_fma(-r2, inv, 1.0);
                inv = __builtin_fma(inv, err, inv);
                err = __builtin_fma(-r2, inv, 1.0);
                inv = __builtin_fma(inv, err, inv);
                mi = s.m * inv;
                beta = dw * (-2.0 * inv);
            } else {
                double u = __builtin_amdgcn_rsq(r2);
#pragma unroll
                for (int step = 0; step < 2; step++) {
                    const double err = __builtin_fma(-(r2 * u), u, 1.0);
                    u = __builtin_fma(0.5 * u, err, u);
                }
                const double u2 = u * u;
                mi = (s.m * u) * u2;
                beta = dw * (-3.0 * u2);
            }
            const double ux = __builtin_fma(beta, dx, wx);
            const double uy = __builtin_fma(beta, dy, wy);
            const double uz = __builtin_fma(beta, dz, wz);
            t.ax[k] = __builtin_fma(mi, dx, t.ax[k]);
            t.ay[k] = __builtin_fma(mi, dy, t.ay[k]);
            t.az[k] = __builtin_fma(mi, dz, t.az[k]);
            t.jx[k] = __builtin_fma(mi, ux, t.jx[k]);
            t.jy[k] = __builtin_fma(mi, uy, t.jy[k]);
            t.jz[k] = __builtin_fma(mi, uz, t.jz[k]);
        }
    }
}

// (amdgpu_waves_per_eu: the register allocator's line is K7's 128 VGPRs -- four waves per SIMD -- not the 256 the workgroup size allows)
template <int LAW, int T>
__global__ __launch_bounds__(kTile) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_acc_jerk64(const AccJerk64Src* __restrict__ src, const int* __restrict__ list, const int n_targets, const int n_sources,
                  const int stride, AccJerk64* __restrict__ partial)
{
    constexpr int kBlock = 64 * T;           // targets per workgroup
    __shared__ double red[3][6][kBlock];     // the sums of waves 1 - 3
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t0 = blockIdx.x * kBlock;
    // this workgroup's source range, then this wave's quarter of it, as k_sweep64 cuts them
    // (the first n % S ranges and the first len % 4 quarters are one source longer)
    const int base = n_sources / (int)gridDim.y, rem = n_sources % (int)gridDim.y, sy = (int)blockIdx.y;
    const int j0 = sy * base + (sy < rem ? sy : rem), len = base + (sy < rem ? 1 : 0);
    const int ja = j0 + (len >> 2) * wave + (wave < (len & 3) ? wave : (len & 3));
    const int jb = ja + (len >> 2) + (wave < (len & 3) ? 1 : 0);
    TargetsAJ64<T> t;
#pragma unroll
    for (int k = 0; k < T; k++) {
        int slot = t0 + k * 64 + lane;
        slot = slot < n_targets ? slot : n_targets - 1;   // (idle lanes repeat the last target; nothing of theirs is written)
        const double4* rec = reinterpret_cast<const double4*>(src + (list ? list[slot] : slot));
        const double4 p = rec[0], v = rec[1];
        t.x[k] = p.x; t.y[k] = p.y; t.z[k] = p.z;
        t.vx[k] = v.x; t.vy[k] = v.y; t.vz[k] = v.z;
        t.ax[k] = t.ay[k] = t.az[k] = t.jx[k] = t.jy[k] = t.jz[k] = 0.0;
    }
    sweep_aj64<LAW, T>(src, ja, jb, t);
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < T; k++) {   // target k * 64 + lane of the block: conflict-free rows
            red[wave - 1][0][k * 64 + lane] = t.ax[k];
            red[wave - 1][1][k * 64 + lane] = t.ay[k];
            red[wave - 1][2][k * 64 + lane] = t.az[k];
            red[wave - 1][3][k * 64 + lane] = t.jx[k];
            red[wave - 1][4][k * 64 + lane] = t.jy[k];
            red[wave - 1][5][k * 64 + lane] = t.jz[k];
        }
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int k = 0; k < T; k++) {
        const int slot = t0 + k * 64 + lane;
        if (slot >= n_targets) continue;
        double a[6] = {t.ax[k], t.ay[k], t.az[k], t.jx[k], t.jy[k], t.jz[k]};
#pragma unroll
        for (int w = 0; w < 3; w++) {
#pragma unroll
            for (int q = 0; q < 6; q++) a[q] += red[w][q][k * 64 + lane];
        }
        double4* out = reinterpret_cast<double4*>(partial + ((size_t)blockIdx.y * (size_t)stride + (size_t)slot));
        out[0] = make_double4(a[0], a[1], a[2], 0.0);
        out[1] = make_double4(a[3], a[4], a[5], 0.0);
    }
}

__global__ __launch_bounds__(kTile) void k_reduce_aj64(const int n_targets, const AccJerk64* __restrict__ partial, const int split,
                                                       const int stride, AccJerk64* __restrict__ out)
{
    const int i = blockIdx.x * kTile + threadIdx.x;
    if (i >= n_targets) return;
    AccJerk64 r = partial[i];
    for (int s = 1; s < split; s++) {
        const AccJerk64 q = partial[(size_t)s * (size_t)stride + (size_t)i];
        r.a.x += q.a.x; r.a.y += q.a.y; r.a.z += q.a.z;
        r.j.x += q.j.x; r.j.y += q.j.y; r.j.z += q.j.z;
    }
    out[i] = r;
}

template <int LAW, int T>
void launch_one(const AccJerk64Src* src, const int* list, int n_targets, int n_sources, int split, int stride, AccJerk64* partial,
                hipStream_t stream)
{
    const dim3 grid((unsigned)(stride / (64 * T)), (unsigned)split);
    hipLaunchKernelGGL((k_acc_jerk64<LAW, T>), grid, dim3(kTile), 0, stream, src, list, n_targets, n_sources, stride, partial);
}

template <int LAW>
hipError_t launch_law(const AccJerk64Src* src, const int* list, int n_targets, int n_sources, int split, int t, int stride,
                      AccJerk64* partial, hipStream_t stream)
{
    if (t == 1) launch_one<LAW, 1>(src, list, n_targets, n_sources, split, stride, partial, stream);
    else if (t == 2) launch_one<LAW, 2>(src, list, n_targets, n_sources, split, stride, partial, stream);
    else if (t == 4) launch_one<LAW, 4>(src, list, n_targets, n_sources, split, stride, partial, stream);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

hipError_t launch_widen_aj64(const float4* posm, const float4* vel, AccJerk64Src* src, int n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_widen_aj64, dim3((n + kTile - 1) / kTile), dim3(kTile), 0, stream, posm, vel, src, n);
    return hipGetLastError();
}

int acc_jerk64_targets(int n_targets)
{
    // the full sweep's T while the targets fill its lanes; a list that leaves whole waves' worth of slots idle halves it
    int t = kAccJerk64Targets;
    while (t > 1 && n_targets <= 64 * (t / 2)) t /= 2;
    return t;
}

int acc_jerk64_stride(int n_targets, int t) { return ((n_targets + 64 * t - 1) / (64 * t)) * (64 * t); }

int acc_jerk64_split(int n_targets, int n_sources, int cu_count, int t, int jsplit_opt)
{
    // <= 128 VGPRs: four waves per SIMD, i.e. four workgroups (one wave per SIMD each) resident per CU.  S follows the number of
    // target BLOCKS, without a stop of its own: a list of one block against every source still gives each CU its four workgroups.
    // Every wave keeps 16 sources or more; the grid's y extent ends at 65 535
    const int most = n_sources < 65535 ? (n_sources > 1 ? n_sources : 1) : 65535;
    if (jsplit_opt > 0) return jsplit_opt < most ? jsplit_opt : most;
    const int blocks = acc_jerk64_stride(n_targets, t) / (64 * t);
    const int want = 4 * (cu_count > 0 ? cu_count : 256);
    int s = blocks > 0 ? (want + blocks - 1) / blocks : 1;
    const int cap = n_sources / 64 < 65535 ? n_sources / 64 : 65535;
    s = s < cap ? s : cap;
    return s > 1 ? s : 1;
}

hipError_t launch_acc_jerk64(const AccJerk64Src* src, const int* list, int n_targets, int n_sources, int law, int split, int t,
                             AccJerk64* partial, hipStream_t stream, ForceLaunch* info)
{
    if (n_targets <= 0 || n_sources <= 0) return hipSuccess;
    if (split < 1 || split > 65535 || law < 0 || law > 1) return hipErrorInvalidValue;
    const int stride = acc_jerk64_stride(n_targets, t);
    if (info) *info = ForceLaunch{(stride / (64 * t)) * split, kTile, split, t, 3, 66 + law};
    return law == 1 ? launch_law<1>(src, list, n_targets, n_sources, split, t, stride, partial, stream)
                    : launch_law<0>(src, list, n_targets, n_sources, split, t, stride, partial, stream);
}

hipError_t launch_reduce_aj64(int n_targets, const AccJerk64* partial, int split, int stride, AccJerk64* out, hipStream_t stream)
{
    if (n_targets <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_reduce_aj64, dim3((n_targets + kTile - 1) / kTile), dim3(kTile), 0, stream, n_targets, partial, split, stride, out);
    return hipGetLastError();
}

}  // namespace nbx
