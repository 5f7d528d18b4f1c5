// hermite.hip -- K8: the all-pairs acceleration + jerk sweep and the 4th-order Hermite predictor-corrector around it
// (Makino & Aarseth 1992) behind nbx_step_hermite / nbx_acc_jerk / nbx_hermite_timestep.
//
// Law (the reference's 1/r pair law and its time derivative), d = p_j - p_i, w = v_j - v_i, s = |d|^2 + eps:
//   a_i = sum_j m_j d / s          j_i = sum_j m_j ( w / s - 2 (d.w) d / s^2 )
// The pair j = i is an exact zero in both (d = w = 0); distinct bodies at one position give zero acceleration and the finite
// jerk m_j w / eps; zero-mass padding sources give 0 * (finite) = 0.  So the loop has no index test.
//
//   k_hermite_predict  one thread per source record: (xp, yp, zp, m, vxp, vyp, vzp, 0), 32 bytes, the Taylor prediction of the
//                      body from the kept (a0, j0); without them (first evaluation, nbx_acc_jerk) the plain widening.  Records
//                      n .. n_pad are zero (mass, velocity): the sweep runs over whole tiles.  A wave-uniform index into this
//                      array is ONE s_load_dwordx8 -- the feeding of K1's variant 6 and of K7 -- which is why the record is
//                      32 bytes and not 28.
//   k_hermite_sweep    a workgroup = 4 wave64 that hold the SAME 64 * T targets, T per lane (x, y, z, vx, vy, vz and six
//                      accumulators each: 24 VGPRs of state at T = 2, the measured best of 1, 2, 4), and split the workgroup's
//                      source range four ways.  The source's eight components reach the VALU as SGPR operands: no LDS and no
//                      barrier in the loop, the next record is loaded while this one is evaluated.  Per pair and target (DIM = 3):
//                        6 v_sub      d, w
//                        3 v_fma      s = |d|^2 + eps
//                        1 v_mul + 2 v_fma   d.w
//                        1 v_rcp_f32  inv = 1 / s  (the ONE reciprocal: 1/s^2 never appears -- beta below carries one inv,
//                                                   the accumulation's m_j inv the other)
//                        3 v_mul      mi = m_j inv,  t = -2 inv (exact),  beta = (d.w) t
//                        3 v_fma      u = w + beta d
//                        6 v_fma      a += mi d,  j += mi u
//                      = 24 VALU + 1 transcendental (DIM = 2: 17 + 1; the z instructions are a quarter of the loop).  Scalar
//                      fp32 instructions, not v_pk_*: this unit is built without packed-fp32 (Makefile NOPK, like every unit since
//                      the octree), so T independent chains per lane cover v_rcp_f32's latency instead of two packed pairs.
//                      The four waves' sums meet in LDS once (red[4][6][64 T], 12 KB at T = 2) and are added in wave order.
//                      Grid = (target blocks, S); partial[S][stride] of (a, j) as two float4.
//   k_hermite_correct  one thread per slab body: the S partials in ascending order, then the corrector with unfused multiplies
//                      and adds in the order written below; writes posm, vel and the kept (a0, j0) <- (a1, j1).
//   k_hermite_keep     the same reduction, writing (a, j) only (first evaluation, nbx_acc_jerk).
//   k_hermite_dtmin    min_i |a_i| / |j_i| over the kept (a0, j0): a fixed-order LDS tree per workgroup, then ONE workgroup over
//                      the partials (the pattern of k_conserved64).  Bodies with |j_i| = 0 are skipped; none left: +inf.
// Deterministic: no atomics, every order fixed by the launch shape (n, S, T).
#include "hermite_math.h"

namespace nbx {

namespace {

constexpr int kT = kHermiteTargets;
static_assert(kT == 1 || kT == 2 || kT == 4, "targets per lane: 1, 2 or 4");
constexpr int kBlock = 64 * kT;   // targets per workgroup

// predict == 0: the record of the body as it is.  c2 = dt^2 / 2, c3 = dt^3 / 6 (rounded once, on the host)
//   xp = ((x + dt v) + c2 a0) + c3 j0        vp = (v + dt a0) + c2 j0
__global__ __launch_bounds__(kTile) void k_hermite_predict(const float4* __restrict__ posm, const float4* __restrict__ vel,
                                                           const HermiteAJ* __restrict__ kept, const int n, const int n_pad,
                                                           const int predict, const float dt, const float c2, const float c3,
                                                           HermiteSrc* __restrict__ src)
{
    const int i = blockIdx.x * kTile + threadIdx.x;
    if (i >= n_pad) return;
    HermiteSrc r{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < n) {
        const float4 p = posm[i];
        const float4 v = vel[i];
        r = HermiteSrc{p.x, p.y, p.z, p.w, v.x, v.y, v.z, 0.f};
        if (predict) {
            const HermiteAJ k = kept[i];
            r.x = __fadd_rn(__fadd_rn(__fadd_rn(p.x, __fmul_rn(dt, v.x)), __fmul_rn(c2, k.a.x)), __fmul_rn(c3, k.j.x));
            r.y = __fadd_rn(__fadd_rn(__fadd_rn(p.y, __fmul_rn(dt, v.y)), __fmul_rn(c2, k.a.y)), __fmul_rn(c3, k.j.y));
            r.z = __fadd_rn(__fadd_rn(__fadd_rn(p.z, __fmul_rn(dt, v.z)), __fmul_rn(c2, k.a.z)), __fmul_rn(c3, k.j.z));
            r.vx = __fadd_rn(__fadd_rn(v.x, __fmul_rn(dt, k.a.x)), __fmul_rn(c2, k.j.x));
            r.vy = __fadd_rn(__fadd_rn(v.y, __fmul_rn(dt, k.a.y)), __fmul_rn(c2, k.j.y));
            r.vz = __fadd_rn(__fadd_rn(v.z, __fmul_rn(dt, k.a.z)), __fmul_rn(c2, k.j.z));
        }
    }
    src[i] = r;
}

template <int DIM>
__global__ __launch_bounds__(kTile) void k_hermite_sweep(const HermiteSrc* __restrict__ src, const int lo, const int n_targets,
                                                         const int tiles_total, HermiteAJ* __restrict__ partial, const int stride)
{
    __shared__ float red[4][6][kBlock];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = (int)blockIdx.y, jsplit = (int)gridDim.y;
    const int t0 = (int)blockIdx.x * kBlock;
    // this workgroup's whole tiles of sources, then this wave's quarter of them (a multiple of 64)
    const int j0 = (int)(((unsigned)tiles_total * (unsigned)split) / (unsigned)jsplit) * kTile;
    const int j1 = (int)(((unsigned)tiles_total * (unsigned)(split + 1)) / (unsigned)jsplit) * kTile;
    const int quarter = (j1 - j0) >> 2;
    const int ja = j0 + quarter * wave, jb = ja + quarter;

    float x[kT], y[kT], z[kT], vx[kT], vy[kT], vz[kT];
    float ax[kT], ay[kT], az[kT], jx[kT], jy[kT], jz[kT];
#pragma unroll
    for (int k = 0; k < kT; k++) {
        int it = t0 + k * 64 + lane;
        it = it < n_targets ? it : n_targets - 1;   // (idle lanes repeat the last target; nothing of theirs is written)
        const float4* rec = reinterpret_cast<const float4*>(src + lo + it);
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
            for (int k = 0; k < kT; k++) {
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
    for (int k = 0; k < kT; k++) {   // target k * 64 + lane of the block: conflict-free rows
        red[wave][0][k * 64 + lane] = ax[k]; red[wave][1][k * 64 + lane] = ay[k]; red[wave][2][k * 64 + lane] = az[k];
        red[wave][3][k * 64 + lane] = jx[k]; red[wave][4][k * 64 + lane] = jy[k]; red[wave][5][k * 64 + lane] = jz[k];
    }
    __syncthreads();
    const int it = t0 + tid;
    if (tid < kBlock && it < n_targets) {
        float q[6];
#pragma unroll
        for (int c = 0; c < 6; c++) {
            q[c] = red[0][c][tid];
#pragma unroll
            for (int w = 1; w < 4; w++) q[c] += red[w][c][tid];
        }
        partial[(size_t)split * stride + it] = HermiteAJ{make_float4(q[0], q[1], q[2], 0.f), make_float4(q[3], q[4], q[5], 0.f)};
    }
}

__device__ __forceinline__ HermiteAJ sum_partials(const HermiteAJ* __restrict__ partial, const int jsplit, const int stride,
                                                  const int i)
{
    HermiteAJ r = partial[i];
    for (int s = 1; s < jsplit; s++) {
        const HermiteAJ q = partial[(size_t)s * stride + i];
        r.a.x += q.a.x; r.a.y += q.a.y; r.a.z += q.a.z;
        r.j.x += q.j.x; r.j.y += q.j.y; r.j.z += q.j.z;
    }
    return r;
}

// (the corrector correct_v / correct_x and the ratio |a| / |j|: hermite_math.h, shared with the block step)
__global__ __launch_bounds__(kTile) void k_hermite_correct(float4* __restrict__ posm, const int lo, const int n_targets,
                                                           float4* __restrict__ vel, const HermiteAJ* __restrict__ partial,
                                                           const int jsplit, const int stride, HermiteAJ* __restrict__ kept,
                                                           const float h, const float c12)
{
    const int i = blockIdx.x * kTile + threadIdx.x;
    if (i >= n_targets) return;
    const HermiteAJ n1 = sum_partials(partial, jsplit, stride, i);
    const HermiteAJ n0 = kept[i];
    float4 v = vel[i];
    float4 p = posm[lo + i];
    const float v1x = correct_v(v.x, n0.a.x, n1.a.x, n0.j.x, n1.j.x, h, c12);
    const float v1y = correct_v(v.y, n0.a.y, n1.a.y, n0.j.y, n1.j.y, h, c12);
    const float v1z = correct_v(v.z, n0.a.z, n1.a.z, n0.j.z, n1.j.z, h, c12);
    p.x = correct_x(p.x, v.x, v1x, n0.a.x, n1.a.x, h, c12);
    p.y = correct_x(p.y, v.y, v1y, n0.a.y, n1.a.y, h, c12);
    p.z = correct_x(p.z, v.z, v1z, n0.a.z, n1.a.z, h, c12);
    v.x = v1x; v.y = v1y; v.z = v1z;
    posm[lo + i] = p;
    vel[i] = v;
    kept[i] = n1;
}

__global__ __launch_bounds__(kTile) void k_hermite_keep(const int n_targets, const HermiteAJ* __restrict__ partial,
                                                        const int jsplit, const int stride, HermiteAJ* __restrict__ kept)
{
    const int i = blockIdx.x * kTile + threadIdx.x;
    if (i >= n_targets) return;
    kept[i] = sum_partials(partial, jsplit, stride, i);
}

__device__ __forceinline__ float tree_min(float* red, const int tid, float r)
{
    red[tid] = r;
    __syncthreads();
    for (int half = kTile / 2; half > 0; half >>= 1) {
        if (tid < half) red[tid] = fminf(red[tid], red[tid + half]);
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(kTile) void k_hermite_dtmin(const HermiteAJ* __restrict__ kept, const int n_targets,
                                                         float* __restrict__ block_min)
{
    __shared__ float red[kTile];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kTile + tid;
    float r = __builtin_inff();
    if (i < n_targets) r = hermite_ratio(kept[i]);
    r = tree_min(red, tid, r);
    if (tid == 0) block_min[blockIdx.x] = r;
}

__global__ __launch_bounds__(kTile) void k_hermite_dtmin_last(const float* __restrict__ block_min, const int blocks,
                                                              float* __restrict__ out)
{
    __shared__ float red[kTile];
    const int tid = threadIdx.x;
    float r = __builtin_inff();
    for (int b = tid; b < blocks; b += kTile) r = fminf(r, block_min[b]);
    r = tree_min(red, tid, r);
    if (tid == 0) out[0] = r;
}

}  // namespace

int hermite_stride(int n_targets) { return ((n_targets + kBlock - 1) / kBlock) * kBlock; }

int hermite_split(int n_targets, int tiles_total, int cu_count)
{
    // The reasoning of choose_launch for the wave-split sweep: 32 workgroups per CU (64 where targets are scarce), every wave
    // keeps at least one tile of sources.  Measured (docs/rounds/r09.md): the sweep gains 2 - 4 % from S = 4 up to 64 at
    // 262 144 bodies and loses 5 % at 65 536 with S = 8 instead of 32 -- the longer loop does not want fewer workgroups than K1
    const int blocks = hermite_stride(n_targets) / kBlock;
    const int want = (cu_count > 0 ? cu_count : 256) * (n_targets < 131072 ? 64 : 32);
    int s = 1;
    while (blocks * s < want && s < 64) s *= 2;
    const int cap = tiles_total / 4 > 1 ? tiles_total / 4 : 1;
    return s < cap ? s : cap;
}

hipError_t launch_hermite_predict(const float4* posm, const float4* vel, const HermiteAJ* kept, int n, int n_pad, bool predict,
                                  float dt, HermiteSrc* src, hipStream_t stream)
{
    if (n_pad <= 0) return hipSuccess;
    const float c2 = (float)(0.5 * (double)dt * (double)dt), c3 = (float)((double)dt * (double)dt * (double)dt / 6.0);
    hipLaunchKernelGGL(k_hermite_predict, dim3((n_pad + kTile - 1) / kTile), dim3(kTile), 0, stream, posm, vel, kept, n, n_pad,
                       predict ? 1 : 0, dt, c2, c3, src);
    return hipGetLastError();
}

hipError_t launch_hermite_sweep(const HermiteSrc* src, int lo, int n_targets, int tiles_total, int jsplit, int dim,
                                HermiteAJ* partial, hipStream_t stream, ForceLaunch* info)
{
    if (n_targets <= 0 || tiles_total <= 0) return hipSuccess;
    if (jsplit < 1 || jsplit > tiles_total || jsplit > 65535) return hipErrorInvalidValue;
    const int stride = hermite_stride(n_targets);
    const dim3 grid((unsigned)(stride / kBlock), (unsigned)jsplit);
    if (info) *info = ForceLaunch{(int)(grid.x * grid.y), kTile, jsplit, kT, dim, 40};
    if (dim == 3) hipLaunchKernelGGL(k_hermite_sweep<3>, grid, dim3(kTile), 0, stream, src, lo, n_targets, tiles_total, partial, stride);
    else          hipLaunchKernelGGL(k_hermite_sweep<2>, grid, dim3(kTile), 0, stream, src, lo, n_targets, tiles_total, partial, stride);
    return hipGetLastError();
}

hipError_t launch_hermite_correct(float4* posm, int lo, int n_targets, float4* vel, const HermiteAJ* partial, int jsplit,
                                  HermiteAJ* kept, float dt, hipStream_t stream)
{
    if (n_targets <= 0) return hipSuccess;
    const float c12 = (float)((double)dt * (double)dt / 12.0);
    hipLaunchKernelGGL(k_hermite_correct, dim3((n_targets + kTile - 1) / kTile), dim3(kTile), 0, stream, posm, lo, n_targets, vel,
                       partial, jsplit, hermite_stride(n_targets), kept, 0.5f * dt, c12);
    return hipGetLastError();
}

hipError_t launch_hermite_keep(int n_targets, const HermiteAJ* partial, int jsplit, HermiteAJ* kept, hipStream_t stream)
{
    if (n_targets <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_hermite_keep, dim3((n_targets + kTile - 1) / kTile), dim3(kTile), 0, stream, n_targets, partial, jsplit,
                       hermite_stride(n_targets), kept);
    return hipGetLastError();
}

size_t hermite_dtmin_workspace(int n_targets) { return 1 + (size_t)((n_targets + kTile - 1) / kTile); }

hipError_t launch_hermite_dtmin(const HermiteAJ* kept, int n_targets, float* workspace, hipStream_t stream)
{
    const int blocks = (n_targets + kTile - 1) / kTile;   // (0 bodies: the last kernel alone writes +inf)
    if (blocks > 0) hipLaunchKernelGGL(k_hermite_dtmin, dim3(blocks), dim3(kTile), 0, stream, kept, n_targets, workspace + 1);
    hipLaunchKernelGGL(k_hermite_dtmin_last, dim3(1), dim3(kTile), 0, stream, workspace + 1, blocks, workspace);
    return hipGetLastError();
}

}  // namespace nbx
