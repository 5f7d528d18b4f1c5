// force_newton.hip -- K11: the all-pairs sweep of the Plummer-softened NEWTONIAN law (NBX_OPT_LAW = 1) for gfx950 / MI355X.
//
// Law: a_i = sum_j m_j d (|d|^2 + eps)^(-3/2), d = p_j - p_i, eps = kEps (a softening length of 0.01).  The reference's own law,
// which every other force kernel of the engine evaluates, is the 1/r force of force_tile.hip; this one is opt-in and separate.
//   d    = p_j - p_i                                    3 sub              (2 in 2-D)
//   s    = fma(dz,dz,fma(dy,dy,fma(dx,dx,EPS)))         3 fma              (2)
//   u    = v_rsq_f32(s)                                 1 transcendental   (s >= EPS > 0 always)
//   w    = (m_j u) (u u)                                3 mul              (2 when every mass is the same: u (u u))
//   a   += w * d                                        3 fma              (2)
// = 20 algorithmic flops / interaction (15 in 2-D; the count every all-pairs code quotes for this law: Nyland, Harris & Prins,
// GPU Gems 3, ch. 31).  The pair j = i and distinct bodies at one position contribute w * 0 = an exact zero (w <= m 1e6 is
// finite), zero-mass padding records contribute 0 * finite = 0: no index test in the loop, as in K1.
//
// Feeding and mapping are K1's variants 6 / 7 (force_tile.hip, the measured winner there): sources through the SCALAR cache -- posm[j]
// with a wave-uniform j is one s_load_dwordx4 and the record feeds v_pk_* as SGPR-pair operands, no LDS and no barrier in the loop --,
// 256 threads, every lane holding two packed pairs of targets, the four waves of a workgroup sharing 256 targets and each taking a
// quarter of the workgroup's whole source tiles, the four partial sums meeting in LDS once, added in wave order (deterministic).
// Grid = (target block, source split S) flattened as in launch_force_wave_split; partials float4 [S][stride], so K2
// (launch_integrate) and launch_reduce_forces take them unchanged.
// Per two interactions: 3 v_pk_add + 3 v_pk_fma + 2 v_rsq_f32 + 3 v_pk_mul + 3 v_pk_fma = 12 packed + 2 transcendental (K1: 10 + 2).
// UNIT_MASS (every mass identical, known on the host: min == max): m_j leaves the loop (11 + 2), the common mass multiplies the
// finished sums; sources are then weightless, so the loop ends at the true body count and no pad record is swept.  There is no
// "common mass + exceptions" form here: K2's MassExceptions path recomputes the 1/r law and is never reached under this law.
// One design for every size: no LDS-tile sibling for small systems (what that costs below 16 384 bodies: docs/rounds/r12.md).
#include "kernels.h"

#ifndef NBX_NEWTON_UNROLL
#define NBX_NEWTON_UNROLL 8   // sources per unrolled loop body (the A/B against 4: docs/rounds/r12.md)
#endif

namespace nbx {

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

template <int DIM, int UNROLL, bool UNIT_MASS>
__global__ __launch_bounds__(kTile) void k_newton_pkw(const float4* __restrict__ posm, const int lo, const int n_targets,
                                                      const int tiles_total, const int n_sources, const int jsplit,
                                                      float4* __restrict__ acc_partial, const int acc_stride, const float unit_mass)
{
    constexpr int P = 2;
    __shared__ float red[4][3][kTile];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x % jsplit;
    const int iblk = blockIdx.x / jsplit;
    const int j0 = (int)(((unsigned)tiles_total * (unsigned)split) / (unsigned)jsplit) * kTile;
    const int j1 = (int)(((unsigned)tiles_total * (unsigned)(split + 1)) / (unsigned)jsplit) * kTile;
    const int quarter = (j1 - j0) >> 2;             // whole tiles per workgroup: a multiple of 64
    const int ja = j0 + quarter * wave;
    int jb = ja + quarter;
    if (UNIT_MASS) jb = jb < n_sources ? jb : n_sources;
    v2f xi[P], yi[P], zi[P], ax[P], ay[P], az[P];
#pragma unroll
    for (int p = 0; p < P; p++) {   // (idle lanes repeat the last target; nothing of theirs is written)
        int ia = iblk * kTile + (2 * p) * 64 + lane;
        int ib = ia + 64;
        ia = ia < n_targets ? ia : n_targets - 1;
        ib = ib < n_targets ? ib : n_targets - 1;
        const float4 pa = posm[lo + ia];
        const float4 pb = posm[lo + ib];
        xi[p] = v2f{pa.x, pb.x}; yi[p] = v2f{pa.y, pb.y}; zi[p] = v2f{pa.z, pb.z};
        ax[p] = v2f{0.f, 0.f}; ay[p] = v2f{0.f, 0.f}; az[p] = v2f{0.f, 0.f};
    }
#pragma unroll UNROLL
    for (int j = ja; j < jb; j++) {
        const float4 s = posm[j];
        const v2f sx = {s.x, s.x}, sy = {s.y, s.y}, sz = {s.z, s.z}, sm = {s.w, s.w};
        const v2f eps = {kEps, kEps};
#pragma unroll
        for (int p = 0; p < P; p++) {
            const v2f dx = sx - xi[p];
            const v2f dy = sy - yi[p];
            v2f r2 = __builtin_elementwise_fma(dx, dx, eps);
            r2 = __builtin_elementwise_fma(dy, dy, r2);
            v2f dz = {0.f, 0.f};
            if (DIM == 3) {
                dz = sz - zi[p];
                r2 = __builtin_elementwise_fma(dz, dz, r2);
            }
            v2f u;
            u.x = __builtin_amdgcn_rsqf(r2.x);
            u.y = __builtin_amdgcn_rsqf(r2.y);
            const v2f u2 = u * u;
            const v2f w = (UNIT_MASS ? u : sm * u) * u2;   // m_j u^3: three packed multiplies (two without the mass)
            ax[p] = __builtin_elementwise_fma(w, dx, ax[p]);
            ay[p] = __builtin_elementwise_fma(w, dy, ay[p]);
            if (DIM == 3) az[p] = __builtin_elementwise_fma(w, dz, az[p]);
        }
    }
#pragma unroll
    for (int p = 0; p < P; p++) {   // body b of lane l is target b * 64 + l of the block: conflict-free rows
        red[wave][0][(2 * p) * 64 + lane] = ax[p].x; red[wave][0][(2 * p + 1) * 64 + lane] = ax[p].y;
        red[wave][1][(2 * p) * 64 + lane] = ay[p].x; red[wave][1][(2 * p + 1) * 64 + lane] = ay[p].y;
        red[wave][2][(2 * p) * 64 + lane] = az[p].x; red[wave][2][(2 * p + 1) * 64 + lane] = az[p].y;
    }
    __syncthreads();
    const int it = iblk * kTile + tid;
    if (it < n_targets) {
        float a0 = red[0][0][tid], a1 = red[0][1][tid], a2 = red[0][2][tid];
#pragma unroll
        for (int w = 1; w < 4; w++) { a0 += red[w][0][tid]; a1 += red[w][1][tid]; a2 += red[w][2][tid]; }
        if (UNIT_MASS) { a0 *= unit_mass; a1 *= unit_mass; a2 *= unit_mass; }
        acc_partial[(size_t)split * acc_stride + it] = make_float4(a0, a1, a2, 0.0f);
    }
}

}  // namespace

// the source split of the sweep, chosen as choose_launch does for K1's wave-split variants: the smallest power of two giving 32
// workgroups per CU (64 when targets are scarce), at most 64, every workgroup keeping four source tiles (one per wave)
int newton_split(int n_targets, int tiles_total, int cu_count, int jsplit_opt)
{
    int s = jsplit_opt;
    if (s <= 0) {
        const int iblocks = (n_targets + kTile - 1) / kTile;
        const int want = (cu_count > 0 ? cu_count : 256) * (n_targets < 131072 ? 64 : 32);
        s = 1;
        while (iblocks * s < want && s < 64) s *= 2;
        const int cap = tiles_total / 4 > 1 ? tiles_total / 4 : 1;
        s = s < cap ? s : cap;
    }
    s = s < tiles_total ? s : tiles_total;
    return s > 1 ? s : 1;
}

hipError_t launch_force_newton(const float4* posm, int lo, int n_targets, int tiles_total, int n_sources, int jsplit, int dim,
                               bool unit_mass, float mass, float4* acc_partial, int acc_stride, hipStream_t stream, ForceLaunch* info)
{
    if (n_targets <= 0 || tiles_total <= 0) return hipSuccess;
    if (jsplit < 1) jsplit = 1;
    if (jsplit > tiles_total) jsplit = tiles_total;
    const int iblocks = (n_targets + kTile - 1) / kTile;
    if (acc_stride < n_targets) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(iblocks * jsplit));
    if (info) *info = ForceLaunch{(int)grid.x, kTile, jsplit, 4, dim, unit_mass ? 31 : 30};
#define NBX_NW(DD, UM) \
    hipLaunchKernelGGL((k_newton_pkw<DD, NBX_NEWTON_UNROLL, UM>), grid, dim3(kTile), 0, stream, posm, lo, n_targets, tiles_total, \
                       n_sources, jsplit, acc_partial, acc_stride, mass)
    if (dim == 3) { if (unit_mass) NBX_NW(3, true); else NBX_NW(3, false); }
    else          { if (unit_mass) NBX_NW(2, true); else NBX_NW(2, false); }
#undef NBX_NW
    return hipGetLastError();
}

}  // namespace nbx
