// bh_oct_walk.hip -- the walk of the 3-D Barnes-Hut path (NBX_OPT_BH_DIM = 3).  COMPILED WITH -ffp-contract=off.
//
// Node::compute_force (nbody.rs:333-377) with z added, organised like the child-group walk of the quadtree (bh_walk.hip), widened to
// eight children and three components:
//   * the unit of the walk is an OPENED node: k_oct_groups re-lays the octree as one 192-byte record per interior node holding its
//     children's (x, y, z, m) -- two 16-dword scalar loads -- their thresholds T and their child words (kernels.h OctGroup), in
//     depth-first order, so descending into a node's first opened child is a step to the next record;
//   * the opening test is one compare, dist_sq > T, with T = bh_take_threshold(s, theta): the reference's s / sqrt(dist_sq) < theta
//     exactly (bh_threshold.h), dist_sq = (dx*dx + dy*dy) + dz*dz unfused in that order; a leaf (T = -1) is always evaluated;
//   * one walk per WAVE over 64 bodies in key order: the records arrive through wave-uniform (scalar) loads, who is inside a subtree
//     is a 64-bit lane mask that travels with the walk, the pair law a += m d / (dist_sq + EPS) (v_rcp_f32, the fast class) runs under
//     the mask of the lanes that take the child, the others open it;
//   * opened children go on a wave-level stack, last slot first: lanes of three VGPRs (record, mask lo, mask hi), then LDS for the
//     worst case of 7 pending per level x 21 levels -- the stack cannot overflow;
//   * order of accumulation: a group's present children in DESCENDING slot order, then the opened subtrees in ASCENDING slot order,
//     depth first -- a lane adds the terms of exactly the groups it is inside, whichever bodies share its wave;
//   * the walk ends the step: kick-drift and the kill box (nbody.rs:453-471 with z: outside +-55 on ANY axis about the viewport
//     origin, z origin 0, all three velocity components are zeroed) on its own bodies -- no other walk reads a body's position from
//     the particle array, the records hold copies.  The forces-only form writes F = m a.
// The loop is the compiler's schedule (a hand-scheduled one is a later A/B); this unit is built without the packed-fp32 instructions.
#include "bh_oct_stack.h"
#include "bh_threshold.h"
#include "kernels.h"

namespace nbx {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v8f __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef int v8i __attribute__((ext_vector_type(8)));

// ---- tree -> groups ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void oct_group_slot(const OctNode nd, const float theta, float4& rec, float& T, int& kid)
{
    rec = make_float4(nd.px, nd.py, nd.pz, nd.m);
    if (nd.interior) {
        T = bh_take_threshold(nd.s, theta);
        kid = nd.rank + 1;
    } else {   // a leaf is always evaluated (nbody.rs:371); the body's own leaf adds m * 0 / (0 + EPS) = exactly 0
        T = -1.0f;
        kid = kOctLeaf;
    }
}

__global__ __launch_bounds__(kTile) void k_oct_groups(const OctNode* __restrict__ nodes, const int n_nodes, const float theta,
                                                      OctGroup* __restrict__ groups)
{
    const int k = blockIdx.x * kTile + threadIdx.x;
    if (k >= n_nodes) return;
    const OctNode self = nodes[k];
    if (k != 0 && !self.interior) return;
    OctGroup g;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        g.c[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        g.T[c] = __builtin_inff();   // never taken, and never visited: its child word says absent
        g.kid[c] = kOctAbsent;
    }
    if (k == 0) {   // record 0: the root alone (the reference tests the root like any other node, nbody.rs:338-345)
        OctGroup r = g;
        oct_group_slot(self, theta, r.c[0], r.T[0], r.kid[0]);
        groups[0] = r;
        if (!self.interior) return;
    }
    int c = k + 1;
#pragma unroll
    for (int slot = 0; slot < 8; slot++) {
        if (c < self.skip) {
            const OctNode nd = nodes[c];
            oct_group_slot(nd, theta, g.c[slot], g.T[slot], g.kid[slot]);
            c = nd.skip;
        }
    }
    groups[self.rank + 1] = g;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------
// One child (slot c = record half G, quarter j): the lanes of M with "not (dist_sq <= T)" take it -- a NaN takes (and poisons the sum,
// as in the reference) instead of opening; the pair law runs under their exec mask (the empty asm keeps the block a branch); the
// other lanes of M open it: its record goes on the stack with their mask.
#define NBX_OCT_CHILD(G, j, c)                                                             \
    if (K[c] != kOctAbsent) {                                                              \
        const v2f nxy = {G[4 * (j) + 0], G[4 * (j) + 1]};                                  \
        const v2f d = nxy - p;                                                             \
        const float dz = G[4 * (j) + 2] - pz;                                              \
        const v2f sq = d * d;                                                              \
        const float d2 = (sq.x + sq.y) + dz * dz;                                          \
        const u64 tm = __ballot(!(d2 <= T[c])) & M;                                        \
        if (__builtin_amdgcn_inverse_ballot_w64(tm)) {                                     \
            asm volatile("");                                                              \
            const float s = G[4 * (j) + 3] * __builtin_amdgcn_rcpf(d2 + kEps);             \
            const v2f ss = {s, s};                                                         \
            acc = __builtin_elementwise_fma(ss, d, acc);                                   \
            az = __builtin_fmaf(s, dz, az);                                                \
        }                                                                                  \
        const u64 om = M & ~tm;                                                            \
        if (om != 0ull) st.push(K[c], om, spill);                                          \
    }

__device__ __forceinline__ void oct_walk(const OctGroup* __restrict__ groups, const v2f p, const float pz, u64 M, volatile int* spill,
                                         v2f& acc, float& az)
{
    OctStack st;
    int g = 0;   // record index
    for (;;) {
        // (constant address space: a uniform load from it is a scalar load -- the records were written by an earlier kernel)
        typedef const v16f __attribute__((address_space(4))) * rec16_t;
        typedef const v8f __attribute__((address_space(4))) * rec8f_t;
        typedef const v8i __attribute__((address_space(4))) * rec8i_t;
        const uintptr_t rec = reinterpret_cast<uintptr_t>(groups) +
                              (uintptr_t)(unsigned)__builtin_amdgcn_readfirstlane(g) * (uintptr_t)sizeof(OctGroup);
        const v16f A = *reinterpret_cast<rec16_t>(rec);
        const v16f B = *reinterpret_cast<rec16_t>(rec + 64);
        const v8f T = *reinterpret_cast<rec8f_t>(rec + 128);
        const v8i K = *reinterpret_cast<rec8i_t>(rec + 160);
        if (K[4] != kOctAbsent) {   // (present children come first: nothing behind an absent slot)
            NBX_OCT_CHILD(B, 3, 7)
            NBX_OCT_CHILD(B, 2, 6)
            NBX_OCT_CHILD(B, 1, 5)
            NBX_OCT_CHILD(B, 0, 4)
        }
        NBX_OCT_CHILD(A, 3, 3)
        NBX_OCT_CHILD(A, 2, 2)
        NBX_OCT_CHILD(A, 1, 1)
        NBX_OCT_CHILD(A, 0, 0)
        if (st.sp == 0) break;
        st.pop(g, M, spill);
    }
}

template <bool KICK>
__global__ __launch_bounds__(64) void k_oct_walk(float4* posm, const int n, const unsigned* __restrict__ order,
                                                 const OctGroup* __restrict__ groups, float4* __restrict__ sink, const float dt)
{
    __shared__ int spill_mem[3 * kOctSpill];
    // XCD-aware order (as the quadtree's walks): XCD k walks the k-th contiguous eighth of the key-ordered bodies (gridDim.x % 8 == 0)
    const int blk = (int)(blockIdx.x & 7u) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int t = blk * 64 + (int)threadIdx.x;
    const bool valid = t < n;
    const u64 M = __ballot(valid);
    if (M == 0ull) return;
    const int it = valid ? (int)order[t] : 0;
    const float4 pi = posm[it];
    const v2f p = {pi.x, pi.y};
    v2f acc = {0.0f, 0.0f};
    float az = 0.0f;
    oct_walk(groups, p, pi.z, M, spill_mem, acc, az);
    if (!valid) return;
    if (KICK) {   // v += dt a; p += dt v (nbody.rs:453-464 with z), then the kill box
        float4 v = sink[it];
        float4 q = pi;
        v.x = __fadd_rn(v.x, __fmul_rn(dt, acc.x));
        v.y = __fadd_rn(v.y, __fmul_rn(dt, acc.y));
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
        sink[it] = make_float4(pi.w * acc.x, pi.w * acc.y, pi.w * az, 0.0f);
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
hipError_t launch_oct_groups(const OctNode* nodes, int n_nodes, float theta, OctGroup* groups, hipStream_t stream)
{
    if (n_nodes <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_oct_groups, dim3((unsigned)((n_nodes + kTile - 1) / kTile)), dim3(kTile), 0, stream, nodes, n_nodes, theta, groups);
    return hipGetLastError();
}

hipError_t launch_oct_walk(float4* posm, int n, const unsigned* order, const OctGroup* groups, float4* forces, float4* kick_vel,
                           float dt, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const unsigned walks = (unsigned)(((n + 63) / 64 + 7) / 8 * 8);
    if (kick_vel) hipLaunchKernelGGL(k_oct_walk<true>, dim3(walks), dim3(64), 0, stream, posm, n, order, groups, kick_vel, dt);
    else hipLaunchKernelGGL(k_oct_walk<false>, dim3(walks), dim3(64), 0, stream, posm, n, order, groups, forces, dt);
    return hipGetLastError();
}

}  // namespace nbx
