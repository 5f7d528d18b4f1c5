// kernels.h -- launch wrappers of the gfx950 kernels (internal; the public ABI is include/nbody_mi355x.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nbx {

constexpr int kTile = 256;   // sources per LDS tile == threads per workgroup (4 wave64)
constexpr float kEps = 0.0001f;  // nbody.rs:17

// Flattened Barnes-Hut node (pre-order, skip pointers). 32 bytes, two 16-B loads.
struct BhNode {
    float px, py, m, s;      // COM / particle position, mass, x-extent (x2-x1; nbody.rs:341)
    int32_t skip;            // index of the next node when this subtree is not opened
    int32_t interior;        // 1 = has children (nbody.rs:338), 0 = exterior (leaf)
    float q;                 // opening threshold of the fast walks: s*s for an interior node, -1 for a leaf, so that
                             // "q < theta^2 * d^2" is the MAC for interior nodes and always true for leaves
    int32_t pad1;            // device build: interior nodes before this one in pre-order (where the fast walk files its child group)
};
inline __host__ __device__ float bh_node_q(float s, bool interior) { return interior ? s * s : -1.0f; }

// Round 4: the fast walk's copy of the tree (bh_walk.hip).  One 80-byte record per OPENED node: the (x, y, m, T) of its up to four
// children -- 64 bytes, one s_load_dwordx16 -- present ones first, in the reference's child order (nbody.rs:295-300), then four
// child words.  T = the opening threshold of bh_threshold.h for an interior child (take <=> dist_sq > T: the reference's
// s/sqrt(dist_sq) < theta exactly), -1 for a leaf (always evaluated), +inf for an absent slot.  kid = BYTE offset of that child's
// own record (>= 0), -1 = leaf, -2 = absent.  Record 0 holds the root; the children of the r-th interior node in pre-order are
// record r + 1 -- the records follow the depth-first order of the walk, a node's first opened child is the next record in memory
// (device-built trees: BhNode::pad1 carries r; host-built trees use r = the node's pre-order index: gaps, never touched).
struct alignas(16) BhGroup {
    float4 c[4];
    int4 kid;
};
size_t bh_groups_count(int node_cap);        // records a tree of node_cap nodes needs
bool bh_groups_addressable(int node_cap);    // their byte offsets fit the 31 bits a child word has
// records from the flattened tree, with the step's theta.  n_nodes_or_cap = the node count, or (gated: the count is still on the
// device, bh_gate.h) the capacity of the node array -- the kernel then reads the count itself
// compact: the interior nodes carry their pre-order rank among interior nodes in pad1 (device build)
hipError_t launch_bh_groups(const BhNode* nodes, int n_nodes_or_cap, float theta, BhGroup* groups, bool compact, hipStream_t stream,
                            int* gate_counters = nullptr, int gate_node_cap = 0, int gate_crowd_limit = 0, int gate_queue_limit = 0);
// accelerations of the slab's bodies (fast mode).  wave && perm: one walk per wave (bodies in the spatial order perm; hand_scheduled:
// the assembly loop, else the compiler's), else one per lane; bit-identical results whichever runs
// kick (optional, wave form only): the kick-drift of the step (nbody.rs:453-471, what k_integrate_f2 does) applied by the walk itself
// as soon as a body's acceleration is complete -- legitimate because a walk reads no other body's position from posm (the group
// records hold copies) -- so a small system's step is one dependent kernel shorter.  out is not written then.  host_out: see BuildGate.
struct BhKick {
    float4* vel;      // [n_targets] this slab's velocities; nullptr = no kick (the walk writes accelerations to out)
    float4* posm;     // the same array the walk reads its bodies from
    float dt;         // (the reference's velocity kill outside +-55, nbody.rs:466-471, is always applied: this is the Barnes-Hut step)
    int* host_out;    // gated step: pinned words the build's counters are handed to (nullptr: none)
    float4* sorted;   // optional [n_targets]: the new positions once more, in the order the walks took the bodies (entry t = body
                      // perm[t]): the next build's sort walks the bodies in exactly that order and reads them from here, coalesced,
                      // instead of gathering 16 MB of random 16-byte records (round 5)
};
hipError_t launch_bh_walk_groups(const float4* posm, int lo, int n_targets, const BhGroup* groups, float2* out, hipStream_t stream,
                                 const unsigned* perm, bool wave, bool hand_scheduled, int* gate_counters = nullptr,
                                 int gate_node_cap = 0, int gate_crowd_limit = 0, int gate_queue_limit = 0,
                                 unsigned long long* trace = nullptr, const BhKick* kick = nullptr);
// trace (optional, 4 words per walk = workgroup): s_memrealtime (10 ns ticks) at its start and end, groups loaded (bit 31: redone with the LDS spill) | chunk << 32, HW_ID | XCC_ID << 32
int bh_walk_count(int n_targets, int* bodies_per_walk = nullptr);   // walks (workgroups) of the wave form, a multiple of 8
hipError_t launch_bh_count_groups(const float4* posm, int lo, int n_targets, const BhGroup* groups, unsigned long long* totals,
                                  hipStream_t stream);   // totals[0] children visited, [1] pair laws, [2] opening tests (visits of
                                                         // interior nodes), [3] groups loaded (per body)
hipError_t launch_bh_thresholds(const float* s, const float* theta, float* out, int count, hipStream_t stream);   // test hook

// ---- 3-D Barnes-Hut (NBX_OPT_BH_DIM = 3): the octree built on the device (bh_oct.hip) and walked once per wave (bh_oct_walk.hip) ----
constexpr int kOctLevels = 21;   // 63-bit keys, 3 bits per level
// pre-order record, empty children dropped (what nbx_bh_oct_dump returns): 32 bytes
struct OctNode {
    float px, py, pz, m;     // centre of mass (a single-body leaf: the body itself) and mass
    float s;                 // x-extent of the node's box (the reference's opening test uses x alone, nbody.rs:341)
    int32_t skip;            // slot behind the node's subtree
    int32_t interior;        // 1 = has children
    int32_t rank;            // interior nodes before this one in pre-order (where k_oct_groups files its children); 0 for a leaf
};
// One record per OPENED node, in depth-first order: record r + 1 = the children of the r-th interior node, record 0 = the root alone.
// 8 x (x, y, z, m) = two 16-dword loads, then 8 thresholds T (bh_threshold.h; -1 = leaf: always evaluated, +inf = absent) and 8 child
// words (>= 0: index of the child's own record, kOctLeaf, kOctAbsent).  Present children first, in child-index order.
constexpr int kOctLeaf = -1, kOctAbsent = -2;
struct alignas(64) OctGroup {
    float4 c[8];
    float T[8];
    int32_t kid[8];
};
static_assert(sizeof(OctNode) == 32 && sizeof(OctGroup) == 192, "layouts shared with the kernels and the dump");
// build counters the host reads between the two halves: [0] nodes, [1] leaves, [2] multi-body leaves whose bodies are not within EPS
// of each other (a root box so large that a level-21 cell is wider than EPS: the analogue of the reference's depth panic), [3] depth
size_t oct_workspace_bytes(int n, size_t* sort_tmp_bytes);
const int* oct_counters(const void* workspace);
const unsigned* oct_order(void* workspace, int n, size_t sort_tmp_bytes);   // body indices in key order (valid after oct_build_scan)
// root box, keys, sort, scans: everything up to the node count
hipError_t oct_build_scan(const float4* posm, int n, void* workspace, size_t sort_tmp_bytes, hipStream_t stream);
// node records (n_nodes = counters[0], read by the host: the node array is sized from it)
hipError_t oct_build_emit(int n, void* workspace, size_t sort_tmp_bytes, int n_nodes, OctNode* nodes, hipStream_t stream);
hipError_t launch_oct_groups(const OctNode* nodes, int n_nodes, float theta, OctGroup* groups, hipStream_t stream);
// one walk per wave over 64 bodies in key order.  kick_vel != nullptr: the walk ends the step (kick-drift and the 3-D kill box on its
// own bodies, posm and kick_vel updated in place); else F = m * a of body i into forces[i]
hipError_t launch_oct_walk(float4* posm, int n, const unsigned* order, const OctGroup* groups, float4* forces, float4* kick_vel,
                           float dt, hipStream_t stream);

// ---- K13: the octree under the Newtonian law (NBX_OPT_LAW = 1, bh_oct_newton.hip): second moments and the walk that uses them ----
// The second moment of an interior node about its STORED fp32 centre c', P = sum_k m_k (r_k - c')(r_k - c')^T over the node's leaves
// taken as point masses at their stored centres (a multi-body leaf has its bodies within EPS on every axis: a point, its own P = 0).
// One OctQuad per OctGroup record at the same index, slots filled as k_oct_groups fills c[]: 8 children x (Pxx, Pyy, Pzz, Pxy, Pxz,
// Pyz, tr P, 0) in fp32, so that one child's moments are a single 8-dword scalar load; leaves and absent slots are zero.
struct alignas(64) OctQuad {
    float q[8][8];
};
static_assert(sizeof(OctQuad) == 256, "layout shared with the kernels");
constexpr int kOctMomDoubles = 10;   // per interior node (by rank), fp64: first moment D (3), P (xx yy zz xy xz yz) about c', mass
// bytes of the moments workspace for `interior` interior nodes: node of every rank, completion stamps, the fp64 moments
size_t oct_moments_bytes(int interior);
// bottom-up, deterministic, no atomics: `depth` sweeps (counters[3]) over the interior nodes; a node's result does not depend on
// scheduling.  Then launch_oct_quads files them as records; launch_oct_moment_rows as one 8-float row per node in pre-order
hipError_t launch_oct_moments(const OctNode* nodes, int n_nodes, int interior, int depth, void* workspace, hipStream_t stream);
hipError_t launch_oct_quads(const OctNode* nodes, int n_nodes, int interior, const void* workspace, OctQuad* quads, hipStream_t stream);
hipError_t launch_oct_moment_rows(const OctNode* nodes, int n_nodes, int interior, const void* workspace, float* rows, hipStream_t stream);
// launch_oct_walk's sibling for the Newtonian law: a += M x r^3 for a leaf, + the quadrupole term of an accepted interior node
// when quads != nullptr (monopole only, and no OctQuad read, when it is null)
hipError_t launch_oct_walk_newton(float4* posm, int n, const unsigned* order, const OctGroup* groups, const OctQuad* quads,
                                  float4* forces, float4* kick_vel, float dt, hipStream_t stream);
// ---- K14 (bh_oct_potential.hip): the potential of that walk: same records, same opening decisions ----
// phi_i = sum over the taken children of -M r (+ 0.5 tr(P) r^3 - 1.5 (x^T P x) r^5 for an interior one when quads != nullptr), plus
// m_i / sqrt(eps) for the body's own leaf: j = i excluded.  Exactly one output: phi[i] (float, body order) or wide[i] = (0, 0, 0,
// (double)phi_i), the record launch_conserved64 reads
hipError_t launch_oct_phi(const float4* posm, int n, const unsigned* order, const OctGroup* groups, const OctQuad* quads, float* phi,
                          double4* wide, hipStream_t stream);

struct ForceLaunch {
    int grid, block, jsplit, bpt, dim, variant;
};

// K1: all-pairs accelerations for slab targets [lo, lo+n_targets) against tiles_total*kTile sources.
// acc_partial: [jsplit][acc_stride] float4 (ax, ay, az, unused).
// Variant 1 (k_force_tile_pk: packed math, sources through LDS tiles), bpt = 2 or 4 targets per thread.
hipError_t launch_force_tile(const float4* posm, int lo, int n_targets, int tiles_total, int jsplit, int bpt,
                             int dim, float4* acc_partial, int acc_stride, hipStream_t stream, ForceLaunch* info);

// K1, variants 6 / 7 (k_force_smem_pkw): the four waves of a workgroup share 256 targets and split the workgroup's source
// range; partial sums meet in LDS, so only `jsplit` slabs are written for 4 * jsplit source ranges. unit_mass: every body
// has mass `mass` (the per-interaction multiply leaves the loop); n_sources = true body count (no padding swept).
// exc_idx / exc_rec (unit_mass only, exc_count > 0): workgroup 0 also copies the source record of body exc_idx[k], with the
// weight (its mass - mass) the sweep leaves out, into exc_rec[k] -- the snapshot K2 / the force readout add afterwards.
// widened (K4, fp16 sources): the sources are read from this float4 array -- the half4 copy widened by launch_widen_half --
// instead of posm (targets stay posm); every target's interaction with its own image is then taken out by K2 / the
// force readout (SelfImage); info->variant = 17 / 18.
hipError_t launch_force_wave_split(const float4* posm, int lo, int n_targets, int tiles_total, int n_sources, int jsplit, int dim,
                                   bool unit_mass, float mass, float4* acc_partial, int acc_stride, hipStream_t stream,
                                   ForceLaunch* info, const int* exc_idx = nullptr, float4* exc_rec = nullptr, int exc_count = 0,
                                   const float4* widened = nullptr);
// K11 (force_newton.hip, k_newton_pkw): the same feeding, mapping and partials for the Newtonian law a_i = sum m_j d s^(-3/2)
// (NBX_OPT_LAW = 1).  unit_mass: EVERY body has mass `mass` (no exceptions: K2 gets the empty MassExceptions).  info->variant = 30
// (general masses) / 31 (one common mass), bpt = 4.  acc_stride >= n_targets.
hipError_t launch_force_newton(const float4* posm, int lo, int n_targets, int tiles_total, int n_sources, int jsplit, int dim,
                               bool unit_mass, float mass, float4* acc_partial, int acc_stride, hipStream_t stream, ForceLaunch* info);
// its source split: jsplit_opt if positive (NBX_OPT_JSPLIT), else chosen as choose_launch does for variants 6 / 7
int newton_split(int n_targets, int tiles_total, int cu_count, int jsplit_opt);
// widened[i] = float4(posh[i]) for i < count: the fp16 source copy as fp32 records, once per step (K4)
hipError_t launch_widen_half(const void* posh, float4* widened, int count, hipStream_t stream);

// K4: the packed sweep with sources read from a half4 (x,y,z,m) copy (8 B/body), targets fp32.
hipError_t launch_force_tile_half(const float4* posm, const void* posh, int lo, int n_targets, int tiles_total,
                                  int jsplit, int bpt, int dim, float4* acc_partial, int acc_stride, hipStream_t stream,
                                  ForceLaunch* info);
float half_image(float v);   // (float)(_Float16)v, on the host: the value a source's fp16 copy carries
// posh[first..first+count) = half(posm[...]) (round to nearest even)
hipError_t launch_pack_half(const float4* posm, void* posh, int first, int count, hipStream_t stream);

// Sources whose mass differs from the common mass of a unit-mass sweep (variant 7): after the sweep gave every source the
// common mass, such a body still owes (m - m_common) * d / (|d|^2 + eps) to every target.  rec[k] = (x, y, z, m - m_common)
// of exceptional body k, SNAPSHOT by the sweep kernel itself (K2 moves bodies in place while it reads these).  count = 0: none.
struct MassExceptions {
    const float4* rec;
    const int* idx;      // body index of every record (a target skips its own)
    int count;
    int dim;
};

// K4 on the wave-split kernels: the sources were a widened fp16 copy (src), so every target's sum holds its interaction with
// its OWN image; K2 / the force readout take it out. unit_mass > 0: the sweep weighted every source with it; else with src.w.
struct SelfImage {
    const float4* src;
    float unit_mass;
    int dim;
};

// K2: reduce partials in fixed order (- the self image, + the exceptional sources), kick-drift, write positions in place.
hipError_t launch_integrate(float4* posm, int lo, int n_targets, float4* vel, const float4* acc_partial,
                            int jsplit, int acc_stride, float dt, hipStream_t stream,
                            MassExceptions exc = MassExceptions{nullptr, nullptr, 0, 3},
                            SelfImage si = SelfImage{nullptr, 0.0f, 3});

// forces-only readout: F_i = m_i * a_i into float4 out[n_targets]
hipError_t launch_reduce_forces(const float4* posm, int lo, int n_targets, const float4* acc_partial, int jsplit,
                                int acc_stride, float4* out, hipStream_t stream,
                                MassExceptions exc = MassExceptions{nullptr, nullptr, 0, 3},
                                SelfImage si = SelfImage{nullptr, 0.0f, 3});

// ---- K7 (diag64.hip): the fp64 all-pairs sweep behind nbx_forces_f64 / nbx_conserved ----
#ifndef NBX_SWEEP64_T
#define NBX_SWEEP64_T 4   // (1 and 2 also build: the A/B of docs/rounds/r08.md compiled diag64.hip with -DNBX_SWEEP64_T=...)
#endif
constexpr int kSweep64Targets = NBX_SWEEP64_T;   // T, targets per lane; a workgroup = 4 waves sharing 64 * T targets
// src64[i] = (double4)posm[i] for i < n: the sources as 32-byte records, one 8-dword scalar load each
hipError_t launch_widen64(const float4* posm, double4* src64, int n, hipStream_t stream);
// the source split that fills `cu_count` CUs: at least one, at most n / 64 (every wave keeps 16 sources or more)
int sweep64_split(int n_targets, int n_sources, int cu_count);
int sweep64_stride(int n_targets);   // records per partial slab: the targets rounded up to whole workgroups
// partial[s][t] = (sum m_j d / (|d|^2 + eps), sum m_j ln(|d|^2 + eps)) over the s-th of `split` source ranges, for targets
// posm[lo + t], t < n_targets; pot = false leaves the logarithm out (.w = 0)
hipError_t launch_sweep64(const float4* posm, const double4* src64, int lo, int n_targets, int n_sources, int split, bool pot,
                          double4* partial, hipStream_t stream, ForceLaunch* info);
// the Newtonian sibling (k_newton64): partial[s][t] = (sum m_j d s^(-3/2), -sum_{j != t} m_j s^(-1/2)), s = |d|^2 + eps; pot = false
// leaves the potential out (.w = 0).  Same split, stride and partials as launch_sweep64; info->variant = 65
hipError_t launch_newton64(const float4* posm, const double4* src64, int lo, int n_targets, int n_sources, int split, bool pot,
                           double4* partial, hipStream_t stream, ForceLaunch* info);
// out[t] = (m_t * sum of the partials' xyz in ascending split order, w_scale * sum of their w): 1/2 for launch_sweep64's sum of
// m_j ln(s), 1 for launch_newton64's
hipError_t launch_reduce64(const float4* posm, int lo, int n_targets, const double4* partial, int split, double4* out,
                           hipStream_t stream, double w_scale = 0.5);
// the 12 sums of nbx_conserved_id over the slab into sums[0..12); workspace: conserved64_workspace(n_targets) doubles
size_t conserved64_workspace(int n_targets);
hipError_t launch_conserved64(const float4* posm, int lo, int n_targets, const float4* vel, const double4* out, double* workspace,
                              double* sums, hipStream_t stream);

// ---- K12 (acc_jerk64.hip): the fp64 acceleration + jerk sweep behind nbx_acc_jerk_f64, both laws, all bodies or a list ----
constexpr int kAccJerk64Targets = 2;   // T of the full sweep, targets per lane (1, 2 and 4 are built; the A/B is in docs/rounds/r13.md)
// source (and target) record of the sweep: the body in doubles, 64 bytes = one 16-dword scalar load
struct alignas(64) AccJerk64Src {
    double x, y, z, m, vx, vy, vz, pad;
};
// (ax, ay, az, 0), (jx, jy, jz, 0): a partial sum of the sweep, or a slot's result
struct alignas(64) AccJerk64 {
    double4 a, j;
};
static_assert(sizeof(AccJerk64Src) == 64 && sizeof(AccJerk64) == 64, "layouts the kernels address as two double4");
// src[i] = (posm[i], vel[i]) widened exactly, for i < n.  Unsharded engines only: vel holds all n bodies
hipError_t launch_widen_aj64(const float4* posm, const float4* vel, AccJerk64Src* src, int n, hipStream_t stream);
int acc_jerk64_targets(int n_targets);          // T for this many targets: kAccJerk64Targets, less for a list that would leave lanes idle
int acc_jerk64_stride(int n_targets, int t);    // slots per partial slab: the targets rounded up to whole workgroups
// the source split: jsplit_opt if positive (NBX_OPT_JSPLIT; at most n_sources), else from the number of target blocks -- four
// workgroups per CU, however few the targets -- with every wave keeping 16 sources or more
int acc_jerk64_split(int n_targets, int n_sources, int cu_count, int t, int jsplit_opt);
// partial[s][slot] = (a, j) of target src[list[slot]] (list == nullptr: src[slot]), slot < n_targets, over the s-th of `split` ranges
// of the n_sources records, under law 0 (1/r) or 1 (Newtonian); t = 1, 2 or 4.  info->variant = 66 + law, jsplit = split, bpt = t
hipError_t launch_acc_jerk64(const AccJerk64Src* src, const int* list, int n_targets, int n_sources, int law, int split, int t,
                             AccJerk64* partial, hipStream_t stream, ForceLaunch* info);
// out[slot] = the partials of the slot in ascending split order
hipError_t launch_reduce_aj64(int n_targets, const AccJerk64* partial, int split, int stride, AccJerk64* out, hipStream_t stream);

// ---- K8 (hermite.hip): the acceleration + jerk sweep behind nbx_step_hermite / nbx_acc_jerk / nbx_hermite_timestep ----
#ifndef NBX_HERMITE_T
#define NBX_HERMITE_T 2   // (1 and 4 also build: the A/B of docs/rounds/r09.md compiled hermite.hip with -DNBX_HERMITE_T=...)
#endif
constexpr int kHermiteTargets = NBX_HERMITE_T;   // T, targets per lane; a workgroup = 4 waves sharing 64 * T targets
// source record of the sweep: the (predicted) body, 32 bytes = one 8-dword scalar load
struct alignas(32) HermiteSrc {
    float x, y, z, m, vx, vy, vz, pad;
};
// (ax, ay, az, 0), (jx, jy, jz, 0): a partial sum of the sweep, or a body's kept (a0, j0)
struct alignas(32) HermiteAJ {
    float4 a, j;
};
// src[i] = body i of posm / vel for i < n, advanced by dt along its kept (a0, j0) when predict (else as it is: kept is not read);
// zero records for n <= i < n_pad.  Unsharded engines only: vel holds all n bodies
hipError_t launch_hermite_predict(const float4* posm, const float4* vel, const HermiteAJ* kept, int n, int n_pad, bool predict,
                                  float dt, HermiteSrc* src, hipStream_t stream);
int hermite_stride(int n_targets);   // records per partial slab: the targets rounded up to whole workgroups
// the source split for auto: enough workgroups to fill `cu_count` CUs, every wave keeping a whole tile of sources
int hermite_split(int n_targets, int tiles_total, int cu_count);
// partial[s][t] = (a, j) of target src[lo + t], t < n_targets, over the s-th of `jsplit` ranges of the tiles_total * kTile sources;
// 1 <= jsplit <= tiles_total.  info->variant = 40, bpt = T
hipError_t launch_hermite_sweep(const HermiteSrc* src, int lo, int n_targets, int tiles_total, int jsplit, int dim,
                                HermiteAJ* partial, hipStream_t stream, ForceLaunch* info);
// partials in ascending order = (a1, j1); the corrector on posm[lo + i], vel[i] with kept[i] = (a0, j0); kept[i] <- (a1, j1)
hipError_t launch_hermite_correct(float4* posm, int lo, int n_targets, float4* vel, const HermiteAJ* partial, int jsplit,
                                  HermiteAJ* kept, float dt, hipStream_t stream);
// kept[i] <- the partials in ascending order; nothing else is written
hipError_t launch_hermite_keep(int n_targets, const HermiteAJ* partial, int jsplit, HermiteAJ* kept, hipStream_t stream);
// workspace[0] = min_i |a_i| / |j_i| over kept[0..n_targets) (|j_i| = 0 skipped; +inf if none); hermite_dtmin_workspace() floats
size_t hermite_dtmin_workspace(int n_targets);
hipError_t launch_hermite_dtmin(const HermiteAJ* kept, int n_targets, float* workspace, hipStream_t stream);

// ---- K9 (hermite_block.hip): Hermite block time steps behind nbx_step_hermite_block / nbx_acc_jerk_subset ----
// Time is integer: a macro-step of dt_max is kHermiteTicks ticks, a body at level l steps kHermiteTicks >> l of them.
constexpr int kHermiteMaxLevel = 20;
constexpr int kHermiteTicks = 1 << kHermiteMaxLevel;
struct HermiteBody {   // per body, beside its kept (a0, j0): the time it stands at and its level
    int t, level;
};
struct HermiteHead {   // what the scheduler tells the host once per block step: ONE 8-byte read
    int t_next, n_active;
};
// per level: dt = dt_max 2^-l and the constants of predictor and corrector, computed in double and rounded once on the host --
// those of launch_hermite_predict / launch_hermite_correct at dt.  tick = dt_max 2^-20.  eta <= 0: levels are frozen
struct HermiteLevels {
    float dt[kHermiteMaxLevel + 1], c2[kHermiteMaxLevel + 1], c3[kHermiteMaxLevel + 1], h[kHermiteMaxLevel + 1], c12[kHermiteMaxLevel + 1];
    float tick, eta;
};
HermiteLevels hermite_levels(float dt_max, float eta);
int hermite_block_targets(int n_active, int n);   // T, targets per lane, of a block of n_active bodies out of n (n_active == n: K8's)
int hermite_block_stride(int n_active, int t);    // list slots per partial slab: the block rounded up to whole workgroups
// the source split of a block: grows until the block's workgroups fill the CUs, every wave keeping a whole tile of sources;
// n_active == n: exactly hermite_split(n, ...)
int hermite_block_split(int n_active, int n, int tiles_total, int cu_count, int t);
size_t hermite_block_workspace(int n);   // ints: the head, then the workgroups' minima and counts
// bt[i] = (0, the level eta |a_i| / |j_i| asks for; eta <= 0: level 0) from the kept pairs
hipError_t launch_block_init_levels(const HermiteAJ* kept, int n, const HermiteLevels& lv, HermiteBody* bt, hipStream_t stream);
// head = (min_i t_i + step_i, number of bodies due then); list[0 .. n_active) = their indices, ascending.  No atomics
hipError_t launch_block_schedule(const HermiteBody* bt, int n, int* workspace, int* list, hipStream_t stream);
// src[i] = body i advanced from its own time t_i to t_next along its kept pair; zero records for n <= i < n_pad
hipError_t launch_block_predict(const float4* posm, const float4* vel, const HermiteAJ* kept, const HermiteBody* bt, int n, int n_pad,
                                int t_next, const HermiteLevels& lv, HermiteSrc* src, hipStream_t stream);
// partial[s][slot] = (a, j) of target src[list[slot]] over the s-th of `jsplit` source ranges, in K8's summation order.
// info->variant = 41, bpt = t (1 or 2)
hipError_t launch_block_sweep(const HermiteSrc* src, const int* list, int n_active, int tiles_total, int jsplit, int dim, int t,
                              HermiteAJ* partial, hipStream_t stream, ForceLaunch* info);
// the corrector on the listed bodies (scattered to posm, vel, kept), t_i = t_next (0 at the end of the macro-step), new level
hipError_t launch_block_correct(float4* posm, float4* vel, HermiteAJ* kept, HermiteBody* bt, const int* list, int n_active,
                                const HermiteAJ* partial, int jsplit, int stride, int t_next, const HermiteLevels& lv, hipStream_t stream);
// out[slot] = the partials of the slot in ascending order; nothing else is written
hipError_t launch_block_keep(int n_active, const HermiteAJ* partial, int jsplit, int stride, HermiteAJ* out, hipStream_t stream);

// ---- K10 (hermite_train.hip): block steps of at most kTrainMaxBlock bodies, enqueued in trains (NBX_OPT_HERMITE_BLOCK_TRAIN) ----
constexpr int kTrainMaxBlock = 64;   // a SMALL block: one wave of corrector threads, 2 KB of target records; also the partials' stride
struct HermiteTrain {   // what the train's cars have done since launch_train_reset, beside the HermiteHead they keep current
    int t_done, steps, finished, pad;   // the time reached, the block steps run, 1 once the block at 2^20 ticks is corrected
    long long evals;                    // sum of the block sizes
};
// G, the workgroups of the sweep = its source split: jsplit if positive, else one per CU; at most one per source tile
int hermite_train_groups(int tiles_total, int cu_count, int jsplit);
hipError_t launch_train_reset(HermiteTrain* train, hipStream_t stream);
// partial[g][slot] (stride kTrainMaxBlock) = (a, j) of body list[slot] over the g-th of `groups` source ranges; sources split across
// lanes, predicted in registers.  head != nullptr: a car -- (t_next, n_active) from *head, bodies predicted from their own times; does
// nothing if n_active > kTrainMaxBlock or train->finished.  head == nullptr: the bodies as they are, `count` <= kTrainMaxBlock
// listed (kept, bt, train unused).  info->variant = 42, jsplit = groups, bpt = 1
hipError_t launch_train_sweep(const float4* posm, const float4* vel, const HermiteAJ* kept, const HermiteBody* bt, int n, int tiles_total,
                              int groups, int dim, const HermiteHead* head, const HermiteTrain* train, const int* list, int count,
                              const HermiteLevels& lv, HermiteAJ* partial, hipStream_t stream, ForceLaunch* info);
// the second half of a car, one workgroup: partials in ascending order, corrector and level rule on the listed bodies, then the NEXT
// block's (t_next, n_active) into *head and its list into `list`; *train updated.  The same no-op rule
hipError_t launch_train_finish(float4* posm, float4* vel, HermiteAJ* kept, HermiteBody* bt, int n, int* list, HermiteHead* head,
                               HermiteTrain* train, const HermiteAJ* partial, int groups, const HermiteLevels& lv, hipStream_t stream);

// strict (bit-exact) pair: ascending j per target, IEEE divide, no contraction. 2-D.
// kernel: 16 or 8 = workgroups of that many waves per 64 targets (term producers + one summing wave), 1 = one thread per body,
// anything else = by size (strict_kernel_choice); info->variant = -(kernel). Results are bit-identical whichever runs.
// guard (optional device word): when given, max|coordinate| of the sources is reduced into it first and the kernel takes
// the short correctly-rounded division whenever that maximum is <= 1e5 -- the caller passes it only if
// strict_fastdiv_ok(min mass, max mass); null = always the compiler's IEEE division. Results are identical either way.
hipError_t launch_force_strict(const float4* posm, int n, int lo, int n_targets, float2* force_out,
                               hipStream_t stream, ForceLaunch* info = nullptr, unsigned* guard = nullptr, int kernel = 0);
int strict_kernel_choice(int n_targets);
bool strict_fastdiv_ok(float mass_min, float mass_max);
// *guard = float bits of max(|x|, |y|, |z|) over posm[0..n_records) (NaN counts as +inf)
hipError_t launch_max_coord(const float4* posm, int n_records, unsigned* guard, hipStream_t stream);
// kick-drift from a per-body force (v += (dt*F)/m, nbody.rs:155) or acceleration (is_accel: v += dt*a),
// optional velocity kill box (nbody.rs:466-471).
// gate_* (optional; see bh_eval.hip BuildGate): the kernel runs only if the device tree build whose counters these are
// produced a usable tree -- for steps enqueued before the host has read the build's outcome
hipError_t launch_integrate_f2(float4* posm, int lo, int n_targets, float4* vel, const float2* force, float dt,
                               int is_accel, int killbox, hipStream_t stream, int* gate_counters = nullptr,
                               int gate_node_cap = 0, int gate_crowd_limit = 0, int gate_queue_limit = 0, int* gate_host_out = nullptr);

// K3: Barnes-Hut traversal. mode 0 = fast (sequential pre-order accumulation, rcp),
// mode 1 = strict (hierarchical summation order of nbody.rs:354-360 via an explicit frame stack,
// IEEE sqrt/divide): bit-exact with the reference traversal.  mode 2 / 3 = the wave-uniform forms of 0 / 1
// (need perm: bodies in a spatial order); same results as 0 / 1.
// perm (optional): thread t evaluates body perm[t] -- a GLOBAL body index inside the slab
// [lo, lo + n_targets) -- instead of body lo + t (spatial order => coherent waves); force_out is indexed by body - lo
// gate_* (fast walks only): as launch_integrate_f2; n_nodes is then read from gate_counters[0] on the device
hipError_t launch_bh_eval(const float4* posm, int lo, int n_targets, const BhNode* nodes, int n_nodes, float theta,
                          int mode, float2* force_out, hipStream_t stream, const unsigned* perm = nullptr,
                          int* gate_counters = nullptr, int gate_node_cap = 0, int gate_crowd_limit = 0,
                          int gate_queue_limit = 0);

// planar (x, y) of posm[0..n) into device-visible pinned host arrays (input of the host quadtree build)
hipError_t launch_split_xy(const float4* posm, int n, float* xs_host_pinned, float* ys_host_pinned, hipStream_t stream);

hipError_t launch_bh_count(const float4* posm, int lo, int n_targets, const BhNode* nodes, int n_nodes, float theta,
                           unsigned long long* totals, hipStream_t stream);

// Quadtree build on the device (bh_build.hip): same node set as the host build, flattened straight into `out`.
size_t device_tree_workspace_bytes(int n, int node_cap, size_t* sort_tmp_bytes);
// call once after every (re)allocation of the workspace, before its first use (clears the header's self-clearing ticket)
hipError_t device_tree_workspace_init(void* workspace, hipStream_t stream);
// warm (round 5): the workspace still holds the order an earlier call (this one or device_tree_build_begin) left for the SAME n
// bodies, give or take a step's motion -- the sort then starts from it (bh_sort.hip: k_sample_rank / k_keys_scatter / k_bucket_sort) instead
// of from scratch; a warm sort whose buckets overflow refuses the build (counters[1], see bh_sort.hip)
// sorted_pos (optional, warm only): posm in the order the workspace holds (entry t = posm[order[t]], as the last fused kick-drift
// left it, BhKick::sorted): the warm sort then reads the bodies from there, coalesced, instead of gathering them
hipError_t device_spatial_order(const float4* posm, int n, void* workspace, size_t workspace_bytes, const unsigned** perm_dev,
                                hipStream_t stream, bool warm = false, const float4* sorted_pos = nullptr);
// Routing + stable scatter for the host quadtree build (see bh_front.hip): top_host = ntop records of (x1, y1, x2, y2,
// first_child, bucket); pbucket_host / events_host / offset_host are pinned, device-visible host arrays of rest ints,
// rest 16-byte insert events and nb + 1 64-bit offsets.  Enqueues on `stream`; the caller waits.
size_t device_route_workspace_bytes(int rest, int ntop, int nb);
hipError_t device_route_and_scatter(const float4* posm, int warm, int rest, const void* top_host, int ntop,
                                    const int* bucket_depth_host, int nb, void* workspace, size_t workspace_bytes,
                                    int* pbucket_host, void* events_host, unsigned long long* offset_host, hipStream_t stream);
// perm restricted to the bodies of one slab [lo, hi), order kept (global body indices); *slab_perm points into workspace
size_t device_slab_order_workspace_bytes(int n);
hipError_t device_slab_order(const unsigned* perm, int n, int lo, int hi, void* workspace, size_t workspace_bytes,
                             const unsigned** slab_perm, hipStream_t stream);
// fold: 0 = interior masses / centres are roundings of exact fp64 sums (own tolerance class); 1 = the reference's f32 running
// fold in arrival order (nbody.rs:303-320), EPS clusters of any size replayed in arrival order: the host tree bit for bit; what
// the replay cannot reproduce reports status 2 (caller builds on the host; the reasons are in the build's counter word 5).
constexpr int kFoldFaithfulMax = 65536;   // bit-exact mode (only this class serves it): faithful fold up to this many bodies (the root's chain is n serial steps)
// Fast mode, default class BY COST (round 6): the reference fold only while its build takes at most 1.5 x the
// exact-sum build's.  Measured (profiles/r06_bh_sizes.jsonl, build ms reference / exact): 2 000 bodies 0.114 / 0.044, 10 000
// 0.19 / 0.057, 65 536 1.09 / 0.086 -- 2.6 x at the smallest size listed and growing (the root's fold is n serial f32 steps), and
// below 1 024 bodies this class is served by the host build anyway: at NO size the device build serves.  0 = never by default;
// NBX_OPT_BH_FOLD = 1 still asks for it at any size.
constexpr int kFoldCostMax = 0;
// side / ev_go / ev_done (optional, fold = 1): a second stream and two events of the same device -- the root's fold then runs
// on `side` from the start of the build, beside everything else (it is the longest chain and needs only the bodies);
// host_counters: pinned words the build's counters are copied to at the end; null = the caller's gated kick-drift
// (launch_integrate_f2 gate_host_out) hands them over instead, no copy command
hipError_t device_tree_build_begin(const float4* posm, int n, void* workspace, size_t workspace_bytes, int node_cap, BhNode* out,
                                   int* host_counters, const unsigned** perm_dev, hipStream_t stream, int fold = 0,
                                   hipStream_t side = nullptr, hipEvent_t ev_go = nullptr, hipEvent_t ev_done = nullptr,
                                   bool depth_panic_guard = false, bool warm = false, const float4* sorted_pos = nullptr);
hipError_t device_tree_build_end(int n, int node_cap, const int* host_counters, int* n_nodes_host, int* status,
                                 hipStream_t stream, int fold = 0);
// the device-side view of the same verdict: where the build's counters live (for launch_bh_eval / launch_integrate_f2 gates)
// and the limits device_tree_build_end applies to counters[1] (left-behind bodies) and counters[2] (queued folds)
int* device_tree_counters(void* workspace);
constexpr int kWhySortOverflow = 1 << 20;   // refusal reason (counter word 5): a bucket of the warm sort outgrew its slots -- the ORDER failed, not the tree
constexpr int kTreePoisonWord = 9;   // device_tree_counters()[9]: set by a gated kick-drift whose build was refused; while it is set
                                     // every gated kernel is a no-op (the host clears it when it redoes the refused step)
void device_tree_limits(int n, int fold, int* crowd_limit, int* queue_limit);

// nb_draw on the device: counts (uint2 per pixel: body hits, tail hits) -> ABGR framebuffer. Particles whose tail octant
// cannot be decided safely on the device (see draw.hip) are appended to amb[0..*amb_count) (capacity n) with their body
// pixel and velocity; their body hit is counted, their tail is the host's to add.
struct DrawAmbiguous {
    int32_t xi, yi;
    float vx, vy;
};
hipError_t launch_draw(const float4* posm, const float4* vel, int n, int w, int h, float x1, float y1, float scalex,
                       float scaley, void* counts, unsigned* fb, unsigned* amb_count, DrawAmbiguous* amb, hipStream_t stream);

}  // namespace nbx
