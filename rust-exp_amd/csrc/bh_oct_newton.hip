// bh_oct_newton.hip -- K13: the octree path under the Newtonian law (NBX_OPT_BH_DIM = 3, NBX_OPT_LAW = 1): the second moments of
// the interior nodes and the walk that evaluates monopole + quadrupole.  COMPILED WITH -ffp-contract=off, no packed fp32.
//
// Same tree (bh_oct.hip), same records and opening test (bh_oct_walk.hip: OctGroup, dist_sq > T), new pair law.  For a target at p
// and a child with stored centre c', mass M and second moment P:  x = c' - p, d2 = (x.x^2 + x.y^2) + x.z^2 unfused, u = d2 + eps,
// r = u^(-1/2) (v_rsq_f32) and
//   leaf (always taken):        a += M x r^3                     -- the body's own leaf: x = 0, an exact zero
//   interior node taken:        a += x (M r^3 - 1.5 tr(P) r^5 + 7.5 (x^T P x) r^7) - 3 r^5 (P x)
//   monopole-only (QUAD = 0):   the leaf formula for every taken child
// The interior formula is the second-order Taylor term of the Plummer-softened kernel m x (|x|^2 + eps)^(-3/2) in the source's
// offset from c', written with the RAW second moment: the traceless form would drop a term eps tr(P).
//
// P = sum_k m_k (r_k - c')(r_k - c')^T about the node's STORED fp32 centre c', over its leaves as point masses at their stored
// centres.  A multi-body leaf has all its bodies within EPS on every axis: it is a point at its stored centre, its own P is 0.  The
// first moment D = sum_k m_k (r_k - c') is the rounding of the centre; the walk ignores it, as the monopole path does.
//
// Moments: bottom-up in fp64, deterministic, no atomics.  Per interior node (by rank) D (3) and P (6) about its own centre and the
// fp64 sum m of its leaves' masses (the record's fp32 mass is a rounding of it: with that one, m_c Delta Delta^T would carry 2^-24
// of a term that cancels between the children).  A child is shifted to the parent's centre by Delta = c'_child - c'_parent, formed
// in double from the two fp32 centres:
//   m_p += m_c,   D_p += D_c + m_c Delta,   P_p += P_c + D_c Delta^T + Delta D_c^T + m_c Delta Delta^T   (children in slot order)
// Every term scales with the node's size, not with its distance from the origin.  Schedule: `depth` sweeps, one thread per interior
// node; a node computes once, in the first sweep that finds all its interior children stamped by an EARLIER sweep (a stamp equal to
// the current sweep's index reads as "not ready", so a value being written is never read); what it computes does not depend on when.
// An interior node of height h (leaves = 0) is done in sweep h, and the root's height is at most the depth the build reports.
//
// Walk: k_oct_walk's wave-per-64-bodies loop.  "The child is a leaf" is wave-uniform (its child word), so the quadrupole
// arithmetic sits behind a scalar branch and runs only for interior children that some lane takes; the moments reach the VALU as
// SGPR operands, like the centres.  A, B, T, K hold 48 SGPRs and a whole OctQuad would be 64 more, so the moments are fetched either
// per child inside that branch (NBX_OCT_QUAD_FETCH = 0: one 8-dword load, its latency exposed) or per half-record before the half's
// children (1: two 16-dword loads that overlap the children's distance tests, paid whether or not anybody takes an interior child).
#include "bh_oct_stack.h"
#include "kernels.h"

#ifndef NBX_OCT_QUAD_FETCH
#define NBX_OCT_QUAD_FETCH 1   // measured the faster one (docs/rounds/r14.md); 0 stays compilable for the A/B
#endif

namespace nbx {

typedef float v8f __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef int v8i __attribute__((ext_vector_type(8)));

// ---- moments -------------------------------------------------------------------------------------------------------------------
struct OctMomWs {
    int* node_of;    // [interior] pre-order index of the interior node of rank r
    int* stamp;      // [interior] 0 = not computed, else the sweep that computed it
    double* mom;     // [interior][kOctMomDoubles]
};
static OctMomWs oct_mom_carve(const void* workspace, int interior, size_t* total = nullptr)
{
    char* w = static_cast<char*>(const_cast<void*>(workspace));
    auto take = [&](size_t b) { char* p = w; w += (b + 255) & ~(size_t)255; return p; };
    OctMomWs k;
    k.node_of = reinterpret_cast<int*>(take(sizeof(int) * (size_t)interior));
    k.stamp = reinterpret_cast<int*>(take(sizeof(int) * (size_t)interior));
    k.mom = reinterpret_cast<double*>(take(sizeof(double) * kOctMomDoubles * (size_t)interior));
    if (total) *total = (size_t)(w - static_cast<char*>(const_cast<void*>(workspace)));
    return k;
}
size_t oct_moments_bytes(int interior)
{
    size_t total = 0;
    (void)oct_mom_carve(nullptr, interior > 0 ? interior : 1, &total);
    return total;
}

__global__ __launch_bounds__(kTile) void k_oct_mom_index(const OctNode* __restrict__ nodes, const int n_nodes, int* __restrict__ node_of,
                                                         int* __restrict__ stamp)
{
    const int k = blockIdx.x * kTile + threadIdx.x;
    if (k >= n_nodes) return;
    const OctNode nd = nodes[k];
    if (!nd.interior) return;
    node_of[nd.rank] = k;
    stamp[nd.rank] = 0;
}

__global__ __launch_bounds__(kTile) void k_oct_mom_sweep(const OctNode* __restrict__ nodes, const int* __restrict__ node_of,
                                                         const int interior, const int sweep, int* stamp, double* mom)
{
    const int r = blockIdx.x * kTile + threadIdx.x;
    if (r >= interior) return;
    if (__atomic_load_n(&stamp[r], __ATOMIC_RELAXED) != 0) return;   // (its own stamp: written by this thread of an earlier sweep)
    const int k = node_of[r];
    const OctNode self = nodes[k];
    for (int c = k + 1, slot = 0; slot < 8 && c < self.skip; slot++) {
        const OctNode nd = nodes[c];
        if (nd.interior) {
            const int s = __atomic_load_n(&stamp[nd.rank], __ATOMIC_RELAXED);
            if (s == 0 || s == sweep) return;   // a child of this sweep may still be writing: the next sweep takes this node
        }
        c = nd.skip;
    }
    double D[3] = {0.0, 0.0, 0.0}, P[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, mass = 0.0;
    for (int c = k + 1, slot = 0; slot < 8 && c < self.skip; slot++) {
        const OctNode nd = nodes[c];
        double Dc[3] = {0.0, 0.0, 0.0}, Pc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, mc = (double)nd.m;
        if (nd.interior) {   // (its mass too: the record's fp32 m is a rounding, and m_c Delta Delta^T cancels between children)
            const double* src = mom + (size_t)nd.rank * kOctMomDoubles;
            for (int a = 0; a < 3; a++) Dc[a] = src[a];
            for (int a = 0; a < 6; a++) Pc[a] = src[3 + a];
            mc = src[9];
        }
        mass += mc;
        const double d[3] = {(double)nd.px - (double)self.px, (double)nd.py - (double)self.py, (double)nd.pz - (double)self.pz};
        const double md[3] = {mc * d[0], mc * d[1], mc * d[2]};
        for (int a = 0; a < 3; a++) D[a] += Dc[a] + md[a];
        // entry (i, j): P_c + (D_c,i Delta_j + Delta_i D_c,j) + (m_c Delta_i) Delta_j, then one addition into the parent's sum
        P[0] += (Pc[0] + (Dc[0] * d[0] + d[0] * Dc[0])) + md[0] * d[0];
        P[1] += (Pc[1] + (Dc[1] * d[1] + d[1] * Dc[1])) + md[1] * d[1];
        P[2] += (Pc[2] + (Dc[2] * d[2] + d[2] * Dc[2])) + md[2] * d[2];
        P[3] += (Pc[3] + (Dc[0] * d[1] + d[0] * Dc[1])) + md[0] * d[1];
        P[4] += (Pc[4] + (Dc[0] * d[2] + d[0] * Dc[2])) + md[0] * d[2];
        P[5] += (Pc[5] + (Dc[1] * d[2] + d[1] * Dc[2])) + md[1] * d[2];
        c = nd.skip;
    }
    double* dst = mom + (size_t)r * kOctMomDoubles;
    for (int a = 0; a < 3; a++) dst[a] = D[a];
    for (int a = 0; a < 6; a++) dst[3 + a] = P[a];
    dst[9] = mass;
    __atomic_store_n(&stamp[r], sweep, __ATOMIC_RELAXED);
}

// (Pxx, Pyy, Pzz, Pxy, Pxz, Pyz, tr P, 0) of a node in fp32: zero for a leaf
__device__ __forceinline__ v8f oct_quad_row(const OctNode nd, const double* __restrict__ mom)
{
    v8f q = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (nd.interior) {
        const double* P = mom + (size_t)nd.rank * kOctMomDoubles + 3;
        for (int a = 0; a < 6; a++) q[a] = (float)P[a];
        q[6] = (float)((P[0] + P[1]) + P[2]);
    }
    return q;
}

__global__ __launch_bounds__(kTile) void k_oct_quads(const OctNode* __restrict__ nodes, const int n_nodes, const double* __restrict__ mom,
                                                     v8f* __restrict__ quads)
{
    const int k = blockIdx.x * kTile + threadIdx.x;
    if (k >= n_nodes) return;
    const OctNode self = nodes[k];
    if (k != 0 && !self.interior) return;
    const v8f zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (k == 0) {   // record 0: the root alone
        quads[0] = oct_quad_row(self, mom);
        for (int slot = 1; slot < 8; slot++) quads[slot] = zero;
        if (!self.interior) return;
    }
    v8f* rec = quads + 8 * ((size_t)self.rank + 1);
    int c = k + 1;
    for (int slot = 0; slot < 8; slot++) {
        v8f q = zero;
        if (c < self.skip) {
            const OctNode nd = nodes[c];
            q = oct_quad_row(nd, mom);
            c = nd.skip;
        }
        rec[slot] = q;
    }
}

__global__ __launch_bounds__(kTile) void k_oct_moment_rows(const OctNode* __restrict__ nodes, const int n_nodes,
                                                           const double* __restrict__ mom, v8f* __restrict__ rows)
{
    const int k = blockIdx.x * kTile + threadIdx.x;
    if (k >= n_nodes) return;
    rows[k] = oct_quad_row(nodes[k], mom);
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------
// One child (slot c = record half G, quarter j), as NBX_OCT_CHILD of bh_oct_walk.hip: the lanes of M with "not (dist_sq <= T)" take
// it under their exec mask, the others open it.  Q(i) names the i-th float of the child's moments: scalar registers.
#if NBX_OCT_QUAD_FETCH == 0
#define NBX_OCT_QUAD_LOAD(c) const v8f Qc = *reinterpret_cast<rec8f_t>(qrec + 32 * (c));
#define NBX_OCT_QUAD_Q(c, i) Qc[i]
#else
#define NBX_OCT_QUAD_LOAD(c)
#define NBX_OCT_QUAD_Q(c, i) (((c) & 2) ? Q1[8 * ((c) & 1) + (i)] : Q0[8 * ((c) & 1) + (i)])
#endif

#define NBX_OCT_NEWTON_CHILD(G, j, c)                                                                          \
    if (K[c] != kOctAbsent) {                                                                                  \
        const float dx = G[4 * (j) + 0] - px;                                                                  \
        const float dy = G[4 * (j) + 1] - py;                                                                  \
        const float dz = G[4 * (j) + 2] - pz;                                                                  \
        const float d2 = (dx * dx + dy * dy) + dz * dz;                                                        \
        const u64 tm = __ballot(!(d2 <= T[c])) & M;                                                            \
        if (__builtin_amdgcn_inverse_ballot_w64(tm)) {                                                         \
            asm volatile("");                                                                                  \
            const float r = __builtin_amdgcn_rsqf(d2 + kEps);                                                  \
            const float r2 = r * r;                                                                            \
            const float r3 = r2 * r;                                                                           \
            const float mono = G[4 * (j) + 3] * r3;                                                            \
            if (QUAD && K[c] != kOctLeaf) {   /* wave-uniform: the child word is a scalar */                   \
                NBX_OCT_QUAD_LOAD(c)                                                                           \
                const float r5 = r3 * r2;                                                                      \
                const float r7 = r5 * r2;                                                                      \
                const float qx = __builtin_fmaf(NBX_OCT_QUAD_Q(c, 4), dz, __builtin_fmaf(NBX_OCT_QUAD_Q(c, 3), dy, NBX_OCT_QUAD_Q(c, 0) * dx)); \
                const float qy = __builtin_fmaf(NBX_OCT_QUAD_Q(c, 5), dz, __builtin_fmaf(NBX_OCT_QUAD_Q(c, 1), dy, NBX_OCT_QUAD_Q(c, 3) * dx)); \
                const float qz = __builtin_fmaf(NBX_OCT_QUAD_Q(c, 2), dz, __builtin_fmaf(NBX_OCT_QUAD_Q(c, 5), dy, NBX_OCT_QUAD_Q(c, 4) * dx)); \
                const float xqx = __builtin_fmaf(dz, qz, __builtin_fmaf(dy, qy, dx * qx));                    \
                const float s = __builtin_fmaf(7.5f * xqx, r7, __builtin_fmaf(-1.5f * NBX_OCT_QUAD_Q(c, 6), r5, mono)); \
                const float w = -3.0f * r5;                                                                    \
                ax += __builtin_fmaf(s, dx, w * qx);                                                           \
                ay += __builtin_fmaf(s, dy, w * qy);                                                           \
                az += __builtin_fmaf(s, dz, w * qz);                                                           \
            } else {                                                                                           \
                ax = __builtin_fmaf(mono, dx, ax);                                                             \
                ay = __builtin_fmaf(mono, dy, ay);                                                             \
                az = __builtin_fmaf(mono, dz, az);                                                             \
            }                                                                                                  \
        }                                                                                                      \
        const u64 om = M & ~tm;                                                                                \
        if (om != 0ull) st.push(K[c], om, spill);                                                              \
    }

template <bool QUAD>
__device__ __forceinline__ void oct_walk_newton(const OctGroup* __restrict__ groups, const OctQuad* __restrict__ quads, const float px,
                                                const float py, const float pz, u64 M, volatile int* spill, float& ax, float& ay,
                                                float& az)
{
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
        (void)qrec;
        const v16f A = *reinterpret_cast<rec16_t>(rec);
        const v16f B = *reinterpret_cast<rec16_t>(rec + 64);
        const v8f T = *reinterpret_cast<rec8f_t>(rec + 128);
        const v8i K = *reinterpret_cast<rec8i_t>(rec + 160);
        if (K[4] != kOctAbsent) {   // (present children come first: nothing behind an absent slot)
#if NBX_OCT_QUAD_FETCH == 1
            v16f Q0 = {}, Q1 = {};
            if (QUAD) { Q0 = *reinterpret_cast<rec16_t>(qrec + 128); Q1 = *reinterpret_cast<rec16_t>(qrec + 192); }
#endif
            NBX_OCT_NEWTON_CHILD(B, 3, 7)
            NBX_OCT_NEWTON_CHILD(B, 2, 6)
            NBX_OCT_NEWTON_CHILD(B, 1, 5)
            NBX_OCT_NEWTON_CHILD(B, 0, 4)
        }
        {
#if NBX_OCT_QUAD_FETCH == 1
            v16f Q0 = {}, Q1 = {};
            if (QUAD) { Q0 = *reinterpret_cast<rec16_t>(qrec); Q1 = *reinterpret_cast<rec16_t>(qrec + 64); }
#endif
            NBX_OCT_NEWTON_CHILD(A, 3, 3)
            NBX_OCT_NEWTON_CHILD(A, 2, 2)
            NBX_OCT_NEWTON_CHILD(A, 1, 1)
            NBX_OCT_NEWTON_CHILD(A, 0, 0)
        }
        if (st.sp == 0) break;
        st.pop(g, M, spill);
    }
}

template <bool KICK, bool QUAD>
__global__ __launch_bounds__(64) void k_oct_walk_newton(float4* posm, const int n, const unsigned* __restrict__ order,
                                                        const OctGroup* __restrict__ groups, const OctQuad* __restrict__ quads,
                                                        float4* __restrict__ sink, const float dt)
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
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    oct_walk_newton<QUAD>(groups, quads, pi.x, pi.y, pi.z, M, spill_mem, ax, ay, az);
    if (!valid) return;
    if (KICK) {   // v += dt a; p += dt v, then the 3-D kill box: k_oct_walk's tail
        float4 v = sink[it];
        float4 q = pi;
        v.x = __fadd_rn(v.x, __fmul_rn(dt, ax));
        v.y = __fadd_rn(v.y, __fmul_rn(dt, ay));
        v.z = __fadd_rn(v.z, __fmul_rn(dt, az));
        q.x = __fadd_rn(q.x, __fmul_rn(dt, v.x));
        q.y = __fadd_rn(q.y, __fmul_rn(dt, v.y));
        q.z = __fadd_rn(q.z, __fmul_rn(dt, v.z));
        const float lim = __fmul_rn(100.0f, 0.55f);
        if (fabsf(__fsub_rn(0.0f, q.x)) > lim || fabsf(__fsub_rn(0.0f, q.y)) > lim || fabsf(__fsub_rn(0.0f, q.z)) > lim) {
            v.x = 0.0f;
            v.y = 0.0f;
            v.z = 0.0f;
        }
        sink[it] = v;
        posm[it] = q;
    } else {
        sink[it] = make_float4(pi.w * ax, pi.w * ay, pi.w * az, 0.0f);
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
hipError_t launch_oct_moments(const OctNode* nodes, int n_nodes, int interior, int depth, void* workspace, hipStream_t stream)
{
    if (n_nodes <= 0 || interior < 0 || interior >= n_nodes) return hipErrorInvalidValue;
    if (interior == 0) return hipSuccess;
    const OctMomWs k = oct_mom_carve(workspace, interior);
    hipLaunchKernelGGL(k_oct_mom_index, dim3((unsigned)((n_nodes + kTile - 1) / kTile)), dim3(kTile), 0, stream, nodes, n_nodes, k.node_of, k.stamp);
    for (int sweep = 1; sweep <= depth; sweep++)
        hipLaunchKernelGGL(k_oct_mom_sweep, dim3((unsigned)((interior + kTile - 1) / kTile)), dim3(kTile), 0, stream, nodes, k.node_of, interior,
                           sweep, k.stamp, k.mom);
    return hipGetLastError();
}

hipError_t launch_oct_quads(const OctNode* nodes, int n_nodes, int interior, const void* workspace, OctQuad* quads, hipStream_t stream)
{
    if (n_nodes <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_oct_quads, dim3((unsigned)((n_nodes + kTile - 1) / kTile)), dim3(kTile), 0, stream, nodes, n_nodes,
                       oct_mom_carve(workspace, interior > 0 ? interior : 1).mom, reinterpret_cast<v8f*>(quads));
    return hipGetLastError();
}

hipError_t launch_oct_moment_rows(const OctNode* nodes, int n_nodes, int interior, const void* workspace, float* rows, hipStream_t stream)
{
    if (n_nodes <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_oct_moment_rows, dim3((unsigned)((n_nodes + kTile - 1) / kTile)), dim3(kTile), 0, stream, nodes, n_nodes,
                       oct_mom_carve(workspace, interior > 0 ? interior : 1).mom, reinterpret_cast<v8f*>(rows));
    return hipGetLastError();
}

template <bool KICK>
static void oct_walk_newton_launch(unsigned walks, float4* posm, int n, const unsigned* order, const OctGroup* groups, const OctQuad* quads,
                                   float4* sink, float dt, hipStream_t stream)
{
    if (quads) hipLaunchKernelGGL((k_oct_walk_newton<KICK, true>), dim3(walks), dim3(64), 0, stream, posm, n, order, groups, quads, sink, dt);
    else hipLaunchKernelGGL((k_oct_walk_newton<KICK, false>), dim3(walks), dim3(64), 0, stream, posm, n, order, groups, quads, sink, dt);
}

hipError_t launch_oct_walk_newton(float4* posm, int n, const unsigned* order, const OctGroup* groups, const OctQuad* quads,
                                  float4* forces, float4* kick_vel, float dt, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const unsigned walks = (unsigned)(((n + 63) / 64 + 7) / 8 * 8);
    if (kick_vel) oct_walk_newton_launch<true>(walks, posm, n, order, groups, quads, kick_vel, dt, stream);
    else oct_walk_newton_launch<false>(walks, posm, n, order, groups, quads, forces, dt, stream);
    return hipGetLastError();
}

}  // namespace nbx
