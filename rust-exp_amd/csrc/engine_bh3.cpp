// engine_bh3.cpp -- the 3-D Barnes-Hut path (NBX_OPT_BH_DIM = 3): octree built on the device (bh_oct.hip), walked once per wave
// (bh_oct_walk.hip; under NBX_OPT_LAW = 1 by bh_oct_newton.hip with the nodes' second moments).  Step, forces-only evaluation, the
// potential of the Newtonian walk with the conserved sums made from it (bh_oct_potential.hip) and the dumps of the tree and its moments.  The build is cold every step and the host reads the
// node count between its two halves (one small synchronous read); the gated asynchronous pipeline, the warm sort, the bit-exact
// mode, sharded and group engines and the fp16 source copy of the quadtree path are not served here: NBX_ERR_STATE.
#include "engine_internal.h"

namespace nbxi {

static constexpr int kOctMaxBodies = 1 << 25;   // node slots are 32-bit and a body can start up to 22 nodes

int bh3_refusal(const nbx_engine* e)
{
    if (e->force_mode != 0) return fail(NBX_ERR_STATE, "NBX_OPT_BH_DIM = 3: the octree path has no bit-exact (strict) mode");
    if (e->world > 1) return fail(NBX_ERR_STATE, "NBX_OPT_BH_DIM = 3: the octree path does not serve a sharded engine (world = %d)", e->world);
    if (e->in_group) return fail(NBX_ERR_STATE, "NBX_OPT_BH_DIM = 3: the octree path does not serve an engine inside an nbx_group");
    if (e->source_half) return fail(NBX_ERR_STATE, "NBX_OPT_BH_DIM = 3: the octree path does not serve the fp16 source copy");
    if (e->n > kOctMaxBodies) return fail(NBX_ERR_STATE, "NBX_OPT_BH_DIM = 3: more than %d bodies", kOctMaxBodies);
    // (the reference asserts a positive mass where it folds one into a node, nbody.rs:304)
    if (e->n > 0 && !(e->mass_min > 0.0f)) return fail(NBX_ERR_TREE, "octree build: a mass is not positive and finite (nbody.rs:304)");
    return NBX_OK;
}

// the octree of the current device state into e->d_oct_nodes; *order = the bodies in key order (device pointer into the workspace)
static int oct_build(nbx_engine* e, int* n_nodes, int* n_leaves, int* depth, const unsigned** order)
{
    HIP_TRY(hipSetDevice(e->device));
    size_t sort_tmp = 0;
    const size_t need = nbx::oct_workspace_bytes(e->n, &sort_tmp);
    if (need > e->oct_ws_bytes) {
        if (e->d_oct_ws) HIP_TRY(hipFree(e->d_oct_ws));
        e->d_oct_ws = nullptr;
        e->oct_ws_bytes = 0;
        HIP_TRY(hipMalloc(&e->d_oct_ws, need + need / 8));
        e->oct_ws_bytes = need + need / 8;
    }
    if (!e->h_oct_counters) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->h_oct_counters), 64, hipHostMallocDefault));
    {
        ProfScope ps(e, NBX_K_TREE_BUILD);
        HIP_TRY(nbx::oct_build_scan(e->d_posm, e->n, e->d_oct_ws, sort_tmp, e->stream));
    }
    HIP_TRY(hipMemcpyAsync(e->h_oct_counters, nbx::oct_counters(e->d_oct_ws), 4 * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(wait_stream(e->stream, e->n <= kSpinMaxBodies));
    const int* c = e->h_oct_counters;
    if (c[2] > 0)
        return fail(NBX_ERR_TREE_DEPTH, "octree: %d leaves of level %d hold bodies further apart than EPS (the root box is too large for %d "
                                        "levels; the reference panics on its depth here, nbody.rs:230-232)", c[2], nbx::kOctLevels, nbx::kOctLevels);
    if (c[0] <= 0 || c[1] <= 0 || c[1] > c[0]) return fail(NBX_ERR_TREE, "octree build: %d nodes, %d leaves for %d bodies", c[0], c[1], e->n);
    // node and group arrays follow the count: no build is refused for pool size
    int rc = grow(&e->d_oct_nodes, &e->oct_nodes_cap, (size_t)c[0] + (size_t)c[0] / 8);
    if (rc != NBX_OK) return rc;
    {
        ProfScope ps(e, NBX_K_TREE_BUILD);
        HIP_TRY(nbx::oct_build_emit(e->n, e->d_oct_ws, sort_tmp, c[0], e->d_oct_nodes, e->stream));
    }
    *n_nodes = c[0];
    *n_leaves = c[1];
    *depth = c[3];
    if (order) *order = nbx::oct_order(e->d_oct_ws, e->n, sort_tmp);
    return NBX_OK;
}

// the second moments of the interior nodes of the tree in e->d_oct_nodes into e->d_oct_mom (bh_oct_newton.hip)
static int oct_moments_sweep(nbx_engine* e, int n_nodes, int interior, int depth)
{
    const int rc = grow(&e->d_oct_mom, &e->oct_mom_cap, nbx::oct_moments_bytes(interior));
    if (rc != NBX_OK) return rc;
    HIP_TRY(nbx::launch_oct_moments(e->d_oct_nodes, n_nodes, interior, depth, e->d_oct_mom, e->stream));
    return NBX_OK;
}

// build, the group (and OctQuad) arrays sized, and with `quad` the moments and their records: everything a walk reads but the group
// records, which depend on theta
static int oct_tree(nbx_engine* e, bool quad, int* n_nodes, int* depth, const unsigned** order)
{
    int leaves = 0;
    int rc = oct_build(e, n_nodes, &leaves, depth, order);
    if (rc != NBX_OK) return rc;
    const size_t records = (size_t)(*n_nodes - leaves) + 1;   // one per interior node + the root's own
    rc = grow(&e->d_oct_groups, &e->oct_groups_cap, records + records / 8);
    if (rc != NBX_OK) return rc;
    if (quad) {
        rc = grow(&e->d_oct_quads, &e->oct_quads_cap, records + records / 8);
        if (rc != NBX_OK) return rc;
        ProfScope ps(e, NBX_K_TREE_BUILD);
        rc = oct_moments_sweep(e, *n_nodes, *n_nodes - leaves, *depth);
        if (rc != NBX_OK) return rc;
        HIP_TRY(nbx::launch_oct_quads(e->d_oct_nodes, *n_nodes, *n_nodes - leaves, e->d_oct_mom, e->d_oct_quads, e->stream));
    }
    return NBX_OK;
}

// build + groups + walk; kick: the walk ends the step, else F = m a into e->d_out4.  Under NBX_OPT_LAW = 1: the moments and their
// records behind the groups (unless NBX_OPT_BH_QUADRUPOLE = 0), then the Newtonian walk
static int oct_evaluate(nbx_engine* e, float theta, bool kick, float dt, int* n_nodes, int* depth)
{
    const unsigned* order = nullptr;
    const bool quad = e->law == 1 && e->bh_quadrupole != 0;
    if (!kick) {
        const int rc = grow(&e->d_out4, &e->out4_cap, (size_t)e->n);
        if (rc != NBX_OK) return rc;
    }
    const int rc = oct_tree(e, quad, n_nodes, depth, &order);
    if (rc != NBX_OK) return rc;
    ProfScope ps(e, NBX_K_BH_EVAL);
    HIP_TRY(nbx::launch_oct_groups(e->d_oct_nodes, *n_nodes, theta, e->d_oct_groups, e->stream));
    if (e->law == 1) {
        HIP_TRY(nbx::launch_oct_walk_newton(e->d_posm, e->n, order, e->d_oct_groups, quad ? e->d_oct_quads : nullptr,
                                            kick ? nullptr : e->d_out4, kick ? e->d_vel : nullptr, dt, e->stream));
        return NBX_OK;
    }
    HIP_TRY(nbx::launch_oct_walk(e->d_posm, e->n, order, e->d_oct_groups, kick ? nullptr : e->d_out4, kick ? e->d_vel : nullptr, dt, e->stream));
    return NBX_OK;
}

// K14 (bh_oct_potential.hip): build + moments + groups + the potential walk, into phi (floats, body order) or wide ((0, 0, 0, phi_i)
// as doubles, what launch_conserved64 reads); exactly one of them.  Enqueued, not waited for
static int oct_potential(nbx_engine* e, float theta, float* phi, double4* wide)
{
    const unsigned* order = nullptr;
    const bool quad = e->bh_quadrupole != 0;
    int nodes = 0, depth = 0;
    const int rc = oct_tree(e, quad, &nodes, &depth, &order);
    if (rc != NBX_OK) return rc;
    ProfScope ps(e, NBX_K_BH_EVAL);
    HIP_TRY(nbx::launch_oct_groups(e->d_oct_nodes, nodes, theta, e->d_oct_groups, e->stream));
    HIP_TRY(nbx::launch_oct_phi(e->d_posm, e->n, order, e->d_oct_groups, quad ? e->d_oct_quads : nullptr, phi, wide, e->stream));
    if (log_enabled())
        std::fprintf(stderr, "[nbx] bh_potential dev=%d n=%d theta=%g nodes=%d depth=%d quad=%d out=%s\n", e->device, e->n, (double)theta, nodes,
                     depth, quad ? 1 : 0, wide ? "f64" : "f32");
    return NBX_OK;
}

// what nbx_bh_potential and nbx_bh_conserved check before their own arguments; on NBX_OK the state is on the device
static int potential_ready(nbx_engine* e, float theta)
{
    if (e->bh_dim != 3)
        return fail(NBX_ERR_STATE, "NBX_OPT_BH_DIM = %d: the tree-walk potential is the octree's (NBX_OPT_BH_DIM = 3)", e->bh_dim);
    if (e->law != 1)
        return fail(NBX_ERR_STATE, "NBX_OPT_LAW = %d: the tree-walk potential serves the Newtonian law (NBX_OPT_LAW = 1); the reference "
                                   "law's 1/2 ln s has another expansion", e->law);
    int rc = bh3_refusal(e);
    if (rc != NBX_OK) return rc;
    if (!(theta > 0.0f) || std::isinf(theta))
        return fail(NBX_ERR_INVALID, "theta must be finite and > 0 (nbx_forces_f64 and nbx_conserved give the all-pairs answer)");
    rc = resolve_pending(e);
    if (rc != NBX_OK) return rc;
    return upload(e);
}

int potential_bh3(nbx_engine* e, float theta, int cap, float* phi)
{
    int rc = potential_ready(e, theta);
    if (rc != NBX_OK) return rc;
    if (cap < e->n) return fail(NBX_ERR_INVALID, "capacity %d < n %d", cap, e->n);
    if (e->n == 0) return 0;
    rc = grow(&e->d_out4, &e->out4_cap, ((size_t)e->n + 3) / 4);   // n floats in the force readout's workspace
    if (rc != NBX_OK) return rc;
    float* d_phi = reinterpret_cast<float*>(e->d_out4);
    rc = oct_potential(e, theta, d_phi, nullptr);
    if (rc != NBX_OK) return rc;
    if (phi) HIP_TRY(hipMemcpyAsync(phi, d_phi, sizeof(float) * (size_t)e->n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return e->n;
}

int conserved_bh3(nbx_engine* e, float theta, int count, double* out)
{
    int rc = potential_ready(e, theta);
    if (rc != NBX_OK) return rc;
    if (count != NBX_CONS_COUNT || !out) return fail(NBX_ERR_INVALID, "count must be NBX_CONS_COUNT (%d) and out non-null", (int)NBX_CONS_COUNT);
    for (int k = 0; k < NBX_CONS_COUNT; k++) out[k] = 0.0;
    if (e->n == 0) return NBX_OK;
    rc = grow(&e->d_out64, &e->out64_cap, (size_t)e->n);
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_cons64, &e->cons64_cap, (size_t)NBX_CONS_COUNT + nbx::conserved64_workspace(e->n));
    if (rc != NBX_OK) return rc;
    rc = oct_potential(e, theta, nullptr, e->d_out64);
    if (rc != NBX_OK) return rc;
    // (world == 1 here: the slab is every body, lo = 0)
    HIP_TRY(nbx::launch_conserved64(e->d_posm, 0, e->n, e->d_vel, e->d_out64, e->d_cons64 + NBX_CONS_COUNT, e->d_cons64, e->stream));
    HIP_TRY(hipMemcpyAsync(out, e->d_cons64, sizeof(double) * NBX_CONS_COUNT, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return NBX_OK;
}

int step_bh3(nbx_engine* e, float theta, float dt)
{
    int rc = bh3_refusal(e);
    if (rc != NBX_OK) return rc;
    rc = resolve_pending(e);
    if (rc != NBX_OK) return rc;
    rc = upload(e);
    if (rc != NBX_OK) return rc;
    if (e->n == 0) return NBX_OK;
    int nodes = 0, depth = 0;
    rc = oct_evaluate(e, theta, /*kick=*/true, dt, &nodes, &depth);
    if (rc != NBX_OK) return rc;   // (NBX_ERR_TREE_DEPTH: nothing behind the scans ran, the state is untouched)
    e->positions_moved();
    e->sort_warm_n = 0;            // the quadtree build's order is of a state this step has left behind
    e->host_pos_valid = false;
    e->host_vel_valid = false;
    if (log_enabled())
        std::fprintf(stderr, "[nbx] step_barnes_hut dev=%d n=%d theta=%g dt=%g mode=fast dim=3 tree=device nodes=%d depth=%d walk=wave law=%d quad=%d\n",
                     e->device, e->n, (double)theta, (double)dt, nodes, depth, e->law, e->law == 1 && e->bh_quadrupole != 0 ? 1 : 0);
    return NBX_OK;
}

int forces_bh3(nbx_engine* e, float theta, float* fx, float* fy, float* fz)
{
    int rc = bh3_refusal(e);
    if (rc != NBX_OK) return rc;
    rc = resolve_pending(e);
    if (rc != NBX_OK) return rc;
    rc = upload(e);
    if (rc != NBX_OK) return rc;
    if (e->n == 0) return 0;
    int nodes = 0, depth = 0;
    rc = oct_evaluate(e, theta, /*kick=*/false, 0.0f, &nodes, &depth);
    if (rc != NBX_OK) return rc;
    std::vector<float4> tmp((size_t)e->n);
    HIP_TRY(hipMemcpyAsync(tmp.data(), e->d_out4, sizeof(float4) * (size_t)e->n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < e->n; i++) {
        if (fx) fx[i] = tmp[(size_t)i].x;
        if (fy) fy[i] = tmp[(size_t)i].y;
        if (fz) fz[i] = tmp[(size_t)i].z;
    }
    return e->n;
}

int oct_dump(nbx_engine* e, void* rows, int cap)
{
    if (e->n > kOctMaxBodies) return fail(NBX_ERR_STATE, "octree: more than %d bodies", kOctMaxBodies);
    int rc = resolve_pending(e);
    if (rc != NBX_OK) return rc;
    rc = upload(e);
    if (rc != NBX_OK) return rc;
    if (e->n == 0) return 0;
    int nodes = 0, leaves = 0, depth = 0;
    rc = oct_build(e, &nodes, &leaves, &depth, nullptr);
    if (rc != NBX_OK) return rc;
    if (rows && cap >= nodes) HIP_TRY(hipMemcpyAsync(rows, e->d_oct_nodes, sizeof(nbx::OctNode) * (size_t)nodes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return nodes;
}

int oct_moments(nbx_engine* e, float* rows, int cap)
{
    if (e->n > kOctMaxBodies) return fail(NBX_ERR_STATE, "octree: more than %d bodies", kOctMaxBodies);
    int rc = resolve_pending(e);
    if (rc != NBX_OK) return rc;
    rc = upload(e);
    if (rc != NBX_OK) return rc;
    if (e->n == 0) return 0;
    int nodes = 0, leaves = 0, depth = 0;
    rc = oct_build(e, &nodes, &leaves, &depth, nullptr);
    if (rc != NBX_OK) return rc;
    if (rows && cap >= nodes) {
        rc = oct_moments_sweep(e, nodes, nodes - leaves, depth);
        if (rc != NBX_OK) return rc;
        rc = grow(&e->d_oct_rows, &e->oct_rows_cap, 8 * (size_t)nodes);
        if (rc != NBX_OK) return rc;
        HIP_TRY(nbx::launch_oct_moment_rows(e->d_oct_nodes, nodes, nodes - leaves, e->d_oct_mom, e->d_oct_rows, e->stream));
        HIP_TRY(hipMemcpyAsync(rows, e->d_oct_rows, sizeof(float) * 8 * (size_t)nodes, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return nodes;
}

}  // namespace nbxi
