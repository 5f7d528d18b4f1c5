// engine_hermite.cpp -- host side of K8 (hermite.hip): nbx_step_hermite, nbx_acc_jerk and nbx_hermite_timestep.
//
// One step of size dt (PEC):  predict every body along its kept (a0, j0)  ->  sweep (a1, j1) at the predicted state  ->  correct,
// keep (a0, j0) <- (a1, j1).  The kept pair and its validity flag (nbx_engine::hermite_valid) are the only state the integrator
// adds; a step that finds the flag clear first evaluates (a0, j0) at the current (x, v): the same sweep behind a zero-length
// prediction.  No kill box, as in nbx_step_brute_force.
#include <limits>

#include "engine_internal.h"

namespace nbxi {

int hermite_sweep_dim(const nbx_engine* e) { return e->dim_opt ? e->dim_opt : (e->any_z ? 3 : 2); }   // as choose_launch

// what the three entry points check first: a device, then a configuration the sweep serves; the upload resolves a Barnes-Hut
// step still in flight (ensure_device)
int hermite_ready(nbx_engine* e)
{
    const int nrc = newton_unserved(e, "the Hermite family (its acceleration + jerk sweeps)");
    if (nrc != NBX_OK) return nrc;
    int rc = ensure_device(e);
    if (rc != NBX_OK) return rc;
    if (e->world > 1) return fail(NBX_ERR_STATE, "the Hermite step serves unsharded engines: the other slabs' velocities are not on this rank");
    if (e->in_group) return fail(NBX_ERR_STATE, "the Hermite step serves single engines, not members of an nbx_group");
    if (e->force_mode != 0) return fail(NBX_ERR_STATE, "the Hermite step has no bit-exact form (NBX_OPT_FORCE_MODE = 1)");
    if (e->source_half) return fail(NBX_ERR_STATE, "the Hermite step reads fp32 sources (NBX_OPT_SOURCE_PRECISION = 16 is set)");
    return upload(e);
}

// predict (dt along the kept pair, or the bodies as they are) and sweep: leaves the partial (a, j) in e->d_hpart
static int predict_and_sweep(nbx_engine* e, bool predict, float dt)
{
    const int n = e->n, tiles_total = e->n_pad / kTile, dim = hermite_sweep_dim(e);
    int split = e->jsplit > 0 ? e->jsplit : nbx::hermite_split(n, tiles_total, e->cu_count);
    split = std::max(1, std::min(split, tiles_total));
    int rc = grow(&e->d_hsrc, &e->hsrc_cap, (size_t)e->n_pad);
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_hpart, &e->hpart_cap, (size_t)split * (size_t)nbx::hermite_stride(n));
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_hkept, &e->hkept_cap, (size_t)n);
    if (rc != NBX_OK) return rc;
    {
        ProfScope ps(e, NBX_K_INTEGRATE);
        HIP_TRY(nbx::launch_hermite_predict(e->d_posm, e->d_vel, e->d_hkept, n, e->n_pad, predict, dt, e->d_hsrc, e->stream));
    }
    ProfScope ps(e, NBX_K_FORCE);
    HIP_TRY(nbx::launch_hermite_sweep(e->d_hsrc, 0, n, tiles_total, split, dim, e->d_hpart, e->stream, &e->last));
    return NBX_OK;
}

// (a0, j0) of the current state into e->d_hkept
int hermite_evaluate_kept(nbx_engine* e)
{
    if (!hermite_kept_usable(e)) e->hblock_valid = false;   // (the levels of a block step belong to the pair that is gone)
    e->hermite_valid = false;
    int rc = predict_and_sweep(e, false, 0.0f);
    if (rc != NBX_OK) return rc;
    HIP_TRY(nbx::launch_hermite_keep(e->n, e->d_hpart, e->last.jsplit, e->d_hkept, e->stream));
    e->hermite_valid = true;
    e->hermite_dim = e->last.dim;
    return NBX_OK;
}

bool hermite_kept_usable(const nbx_engine* e) { return e->hermite_valid && e->hermite_dim == hermite_sweep_dim(e) && e->d_hkept; }

int step_hermite(nbx_engine* e, float dt)
{
    int rc = hermite_ready(e);   // (an upload of new host state takes the flag back: positions_moved())
    if (rc != NBX_OK) return rc;
    if (e->n == 0) return NBX_OK;
    if (!hermite_kept_usable(e)) {
        rc = hermite_evaluate_kept(e);
        if (rc != NBX_OK) return rc;
    }
    e->hermite_valid = false;   // until the corrector is enqueued
    e->hblock_valid = false;    // (a shared step leaves the bodies at one time but its kept pair says nothing about levels)
    rc = predict_and_sweep(e, true, dt);
    if (rc != NBX_OK) return rc;
    {
        ProfScope ps(e, NBX_K_INTEGRATE);
        HIP_TRY(nbx::launch_hermite_correct(e->d_posm, 0, e->n, e->d_vel, e->d_hpart, e->last.jsplit, e->d_hkept, dt, e->stream));
    }
    e->positions_moved();       // (the order-sorted copy of the positions is stale from here) ...
    e->hermite_valid = true;    // ... but the kept pair is the one this step left
    e->hermite_dim = e->last.dim;
    e->host_pos_valid = false;
    e->host_vel_valid = false;
    if (log_enabled())
        std::fprintf(stderr, "[nbx] step_hermite dev=%d n=%d dt=%g variant=%d grid=%d S=%d T=%d dim=%d\n", e->device, e->n, (double)dt,
                     e->last.variant, e->last.grid, e->last.jsplit, e->last.bpt, e->last.dim);
    return NBX_OK;
}

int acc_jerk(nbx_engine* e, int cap, float* ax, float* ay, float* az, float* jx, float* jy, float* jz)
{
    int rc = hermite_ready(e);
    if (rc != NBX_OK) return rc;
    const int n = e->n;
    if (cap < n) return fail(NBX_ERR_INVALID, "capacity %d < particle count %d", cap, n);
    if (n == 0) return 0;
    // always a fresh evaluation: after a Hermite step the kept pair is that of the PREDICTED state, not of the current one
    rc = hermite_evaluate_kept(e);
    if (rc != NBX_OK) return rc;
    std::vector<nbx::HermiteAJ> tmp((size_t)n);
    HIP_TRY(hipMemcpyAsync(tmp.data(), e->d_hkept, sizeof(nbx::HermiteAJ) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < n; i++) {
        if (ax) ax[i] = tmp[i].a.x;
        if (ay) ay[i] = tmp[i].a.y;
        if (az) az[i] = tmp[i].a.z;
        if (jx) jx[i] = tmp[i].j.x;
        if (jy) jy[i] = tmp[i].j.y;
        if (jz) jz[i] = tmp[i].j.z;
    }
    return n;
}

int hermite_timestep(nbx_engine* e, float eta, float* dt_out)
{
    int rc = hermite_ready(e);
    if (rc != NBX_OK) return rc;
    if (!dt_out) return fail(NBX_ERR_INVALID, "null dt_out");
    float ratio = std::numeric_limits<float>::infinity();
    if (e->n > 0) {
        if (!hermite_kept_usable(e)) {
            rc = hermite_evaluate_kept(e);
            if (rc != NBX_OK) return rc;
        }
        rc = grow(&e->d_hdt, &e->hdt_cap, nbx::hermite_dtmin_workspace(e->n));
        if (rc != NBX_OK) return rc;
        HIP_TRY(nbx::launch_hermite_dtmin(e->d_hkept, e->n, e->d_hdt, e->stream));
        HIP_TRY(hipMemcpyAsync(&ratio, e->d_hdt, sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    *dt_out = eta * ratio;
    return NBX_OK;
}

}  // namespace nbxi
