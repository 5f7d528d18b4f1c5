// bh_oct_potential.hip -- K14: the potential of the octree walk under the Newtonian law (NBX_OPT_BH_DIM = 3, NBX_OPT_LAW = 1), behind
// nbx_bh_potential and nbx_bh_conserved.  COMPILED WITH -ffp-contract=off, no packed fp32, as bh_oct_newton.hip.
//
// Same tree, records, moments and opening test as the force walk (bh_oct_newton.hip: OctGroup, OctQuad, "not (dist_sq <= T)" takes
// the child).  For a target at p and a child with stored centre c', mass M and second moment P:  x = c' - p, d2 = (x.x^2 + x.y^2) +
// x.z^2 unfused, u = d2 + eps, r = u^(-1/2) (v_rsq_f32) and
//   leaf (always taken):        phi += -M r
//   interior node taken:        phi += -M r + 0.5 tr(P) r^3 - 1.5 (x^T P x) r^5
//   monopole-only (QUAD = 0):   the leaf formula for every taken child
// The interior formula is the second-order Taylor term of -m (|x + delta|^2 + eps)^(-1/2) in the source's offset delta from c', with
// the RAW second moment: d_i d_j of -(|x|^2 + eps)^(-1/2) is delta_ij r^3 - 3 x_i x_j r^5, half of it contracted with P.  Its
// gradient in x is the force walk's  x (M r^3 - 1.5 tr(P) r^5 + 7.5 (x^T P x) r^7) - 3 r^5 (P x)  term by term.
//
// x^T P x needs no vector P x:  Pxx x^2 + Pyy y^2 + Pzz z^2 + 2 (Pxy xy + Pxz xz + Pyz yz), and the squares are the unfused products
// d2 is made of, so the branch behind "the child is interior" is five FMAs on moments, three products, r^3, r^5 and two FMAs.
//
// Own share: the walk takes the body's own leaf like any other (x = 0 for a one-body leaf: -m_i / sqrt(eps)), so the readout adds
// m_i v_rsq_f32(eps) once and phi_i excludes j = i, as nbx_forces_f64's does.  For a member of a multi-body leaf that treats the
// body's offset from the leaf's centre as zero: all bodies of such a leaf lie within EPS per axis (|x|^2 < 3 EPS^2), and the share is
// wrong by at most |x|^2 / (2 eps) of itself, 1.5e-4 * 100 m_i -- the leaf merge's own approximation.
//
// Walk: one wave per 64 key-ordered bodies, XCD-aware block order, OctStack with its LDS spill area: k_oct_walk_newton's loop with
// one accumulator per lane.  A, B, T, K and the moments are scalar loads from the constant address space and reach the VALU as SGPR
// operands; the body's index and position are the only vector loads.  The moments are fetched per half-record before the half's
// children, two 16-dword loads that overlap the children's distance tests: measured faster than one 8-dword load per interior child
// inside the branch (docs/rounds/r16.md), as in the force walk.
#include "bh_oct_stack.h"
#include "kernels.h"

namespace nbx {

typedef float v8f __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef int v8i __attribute__((ext_vector_type(8)));

// Q(i) names the i-th float of child c's moments (Pxx, Pyy, Pzz, Pxy, Pxz, Pyz, tr P, 0): scalar registers
#define NBX_OCT_PHI_Q(c, i) (((c) & 2) ? Q1[8 * ((c) & 1) + (i)] : Q0[8 * ((c) & 1) + (i)])

// One child (slot c = record half G, quarter j): the lanes of M with "not (dist_sq <= T)" take it under their exec mask, the
// others open it.  d2 is the force walk's, bit for bit: both walks take the same nodes.
#define NBX_OCT_PHI_CHILD(G, j, c)                                                                             \
    if (K[c] != kOctAbsent) {                                                                                  \
        const float dx = G[4 * (j) + 0] - px;                                                                  \
        const float dy = G[4 * (j) + 1] - py;                                                                  \
        const float dz = G[4 * (j) + 2] - pz;                                                                  \
        const float xx = dx * dx, yy = dy * dy, zz = dz * dz;                                                  \
        const float d2 = (xx + yy) + zz;                                                                       \
        const u64 tm = __ballot(!(d2 <= T[c])) & M;                                                            \
        if (__builtin_amdgcn_inverse_ballot_w64(tm)) {                                                         \
            asm volatile("");                                                                                  \
            const float r = __builtin_amdgcn_rsqf(d2 + kEps);                                                  \
            if (QUAD && K[c] != kOctLeaf) {   /* wave-uniform: the child word is a scalar */                   \
                const float r2 = r * r;                                                                        \
                const float r3 = r2 * r;                                                                       \
                const float r5 = r3 * r2;                                                                      \
                const float diag = __builtin_fmaf(NBX_OCT_PHI_Q(c, 2), zz, __builtin_fmaf(NBX_OCT_PHI_Q(c, 1), yy, NBX_OCT_PHI_Q(c, 0) * xx)); \
                const float off = __builtin_fmaf(NBX_OCT_PHI_Q(c, 5), dy * dz, __builtin_fmaf(NBX_OCT_PHI_Q(c, 4), dx * dz, NBX_OCT_PHI_Q(c, 3) * (dx * dy))); \
                const float xqx = __builtin_fmaf(2.0f, off, diag);                                             \
                const float low = __builtin_fmaf(0.5f * NBX_OCT_PHI_Q(c, 6), r3, -(G[4 * (j) + 3] * r));       \
                phi += __builtin_fmaf(-1.5f * xqx, r5, low);                                                   \
            } else {                                                                                           \
                phi = __builtin_fmaf(-G[4 * (j) + 3], r, phi);                                                 \
            }                                                                                                  \
        }                                                                                                      \
        const u64 om = M & ~tm;                                                                                \
        if (om != 0ull) st.push(K[c], om, spill);                                                              \
    }

template <bool QUAD>
__device__ __forceinline__ float oct_walk_phi(const OctGroup* __restrict__ groups, const OctQuad* __restrict__ quads, const float px,
                                              const float py, const float pz, u64 M, volatile int* spill)
{
    float phi = 0.0f;
    OctStack st;
    int g = 0;   // record index
    for (;;) {
        // (constant address space: a uniform load from it is a scalar load -- the records were written by earlier kernels)
        typedef const v16f __attribute__((address_space(4))) * rec16_t;
        typedef const v8f __attribute__((address_space(4))) * rec8f_t;
        typedef const v8i __attribute__((address_space(4))) * rec8i_t;
        const unsigned gi = (unsigned)__builtin_amdgcn_readfirstlane(g);
        const uintptr_t rec = reinterpret_cast<uintptr_t>(groups) + (uintptr_t)gi * (uintptr_t)sizeof(OctGroup);
        const uintptr_t qrec = reinterpret_cast<uintptr_t>(quads) + (uintptr_t)gi * (uintptr_t)sizeof(OctQuad);
        const v16f A = *reinterpret_cast<rec16_t>(rec);
        const v16f B = *reinterpret_cast<rec16_t>(rec + 64);
        const v8f T = *reinterpret_cast<rec8f_t>(rec + 128);
        const v8i K = *reinterpret_cast<rec8i_t>(rec + 160);
        if (K[4] != kOctAbsent) {   // (present children come first: nothing behind an absent slot)
            v16f Q0 = {}, Q1 = {};
            if (QUAD) { Q0 = *reinterpret_cast<rec16_t>(qrec + 128); Q1 = *reinterpret_cast<rec16_t>(qrec + 192); }
            NBX_OCT_PHI_CHILD(B, 3, 7)
            NBX_OCT_PHI_CHILD(B, 2, 6)
            NBX_OCT_PHI_CHILD(B, 1, 5)
            NBX_OCT_PHI_CHILD(B, 0, 4)
        }
        {
            v16f Q0 = {}, Q1 = {};
            if (QUAD) { Q0 = *reinterpret_cast<rec16_t>(qrec); Q1 = *reinterpret_cast<rec16_t>(qrec + 64); }
            NBX_OCT_PHI_CHILD(A, 3, 3)
            NBX_OCT_PHI_CHILD(A, 2, 2)
            NBX_OCT_PHI_CHILD(A, 1, 1)
            NBX_OCT_PHI_CHILD(A, 0, 0)
        }
        if (st.sp == 0) break;
        st.pop(g, M, spill);
    }
    return phi;
}

// WIDE = 0: phi[i] in body order (nbx_bh_potential); 1: wide[i] = (0, 0, 0, (double)phi_i), the record k_conserved64 reads
template <bool QUAD, bool WIDE>
__global__ __launch_bounds__(64) void k_oct_phi(const float4* __restrict__ posm, const int n, const unsigned* __restrict__ order,
                                                const OctGroup* __restrict__ groups, const OctQuad* __restrict__ quads,
                                                float* __restrict__ phi, double4* __restrict__ wide)
{
    __shared__ int spill_mem[3 * kOctSpill];
    // XCD-aware order, as k_oct_walk: XCD k walks the k-th contiguous eighth of the key-ordered bodies (gridDim.x % 8 == 0)
    const int blk = (int)(blockIdx.x & 7u) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int t = blk * 64 + (int)threadIdx.x;
    const bool valid = t < n;
    const u64 M = __ballot(valid);
    if (M == 0ull) return;
    const int it = valid ? (int)order[t] : 0;
    const float4 pi = posm[it];
    const float walked = oct_walk_phi<QUAD>(groups, quads, pi.x, pi.y, pi.z, M, spill_mem);
    if (!valid) return;
    const float own = __builtin_fmaf(pi.w, __builtin_amdgcn_rsqf(kEps), walked);   // the body's own leaf gave -m_i / sqrt(eps)
    if (WIDE) wide[it] = make_double4(0.0, 0.0, 0.0, (double)own);
    else phi[it] = own;
}

hipError_t launch_oct_phi(const float4* posm, int n, const unsigned* order, const OctGroup* groups, const OctQuad* quads, float* phi,
                          double4* wide, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if ((phi == nullptr) == (wide == nullptr)) return hipErrorInvalidValue;   // exactly one output
    const unsigned walks = (unsigned)(((n + 63) / 64 + 7) / 8 * 8);
    if (quads && wide) hipLaunchKernelGGL((k_oct_phi<true, true>), dim3(walks), dim3(64), 0, stream, posm, n, order, groups, quads, phi, wide);
    else if (quads) hipLaunchKernelGGL((k_oct_phi<true, false>), dim3(walks), dim3(64), 0, stream, posm, n, order, groups, quads, phi, wide);
    else if (wide) hipLaunchKernelGGL((k_oct_phi<false, true>), dim3(walks), dim3(64), 0, stream, posm, n, order, groups, quads, phi, wide);
    else hipLaunchKernelGGL((k_oct_phi<false, false>), dim3(walks), dim3(64), 0, stream, posm, n, order, groups, quads, phi, wide);
    return hipGetLastError();
}

}  // namespace nbx
