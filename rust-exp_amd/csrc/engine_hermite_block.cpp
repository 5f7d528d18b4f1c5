// engine_hermite_block.cpp -- host side of K9 (hermite_block.hip): nbx_step_hermite_block, nbx_hermite_block_set_levels /
// nbx_hermite_block_levels, nbx_hermite_kept and nbx_acc_jerk_subset.
//
// A macro-step of dt_max is a chain of block steps.  Each one: the scheduler (t_next, the list of bodies due then) -> ONE 8-byte
// synchronous read of (t_next, n_active), which sizes the grids of what follows -> predict every body to t_next over its own span ->
// sweep (a1, j1) of the listed bodies against all predicted bodies -> correct the listed bodies, choose their new levels.  All
// steps divide the macro-step, so its last block holds every body and leaves them at one time with posm / vel consistent; nothing
// is read after it.  The block state -- (time, level) per body in e->d_hbt -- lives and dies with the kept (a0, j0) of K8
// (nbx_engine::hermite_valid), plus its own flag for what a shared nbx_step_hermite or another dt_max takes away.
// NBX_OPT_HERMITE_BLOCK_TRAIN = L > 0 hands blocks of at most 64 bodies to K10 (hermite_train.hip), L block steps per read:
// train_macro_step below.
#include <cmath>

#include "engine_internal.h"

namespace nbxi {

// T of a block: hermite_block_targets, or NBX_HERMITE_BLOCK_T = 1 | 2 (the A/B of docs/rounds/r10.md); the all-active block keeps K8's
static int block_targets(int n_active, int n)
{
    static const int forced = [] {
        const char* s = std::getenv("NBX_HERMITE_BLOCK_T");
        const int t = s ? std::atoi(s) : 0;
        return t == 1 || t == 2 ? t : 0;
    }();
    return forced && n_active != n ? forced : nbx::hermite_block_targets(n_active, n);
}

// (a, j) of the n_active bodies listed in e->d_hblist against the records in e->d_hsrc: partials in e->d_hpart
static int block_sweep(nbx_engine* e, int n_active, int* stride_out)
{
    const int tiles_total = e->n_pad / kTile, t = block_targets(n_active, e->n);
    int split = e->jsplit > 0 ? e->jsplit : nbx::hermite_block_split(n_active, e->n, tiles_total, e->cu_count, t);
    split = std::max(1, std::min(split, tiles_total));
    const int stride = nbx::hermite_block_stride(n_active, t);
    int rc = grow(&e->d_hpart, &e->hpart_cap, (size_t)split * (size_t)stride);
    if (rc != NBX_OK) return rc;
    ProfScope ps(e, NBX_K_FORCE);
    HIP_TRY(nbx::launch_block_sweep(e->d_hsrc, e->d_hblist, n_active, tiles_total, split, hermite_sweep_dim(e), t, e->d_hpart, e->stream,
                                    &e->last));
    *stride_out = stride;
    return NBX_OK;
}

static int block_buffers(nbx_engine* e)
{
    int rc = grow(&e->d_hbt, &e->hbt_cap, (size_t)e->n);
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_hblist, &e->hblist_cap, (size_t)e->n);
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_hbws, &e->hbws_cap, nbx::hermite_block_workspace(e->n));
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_hsrc, &e->hsrc_cap, (size_t)e->n_pad);
    if (rc != NBX_OK) return rc;
    if (!e->h_hbhead) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->h_hbhead), sizeof(nbx::HermiteHead)));
    return NBX_OK;
}

// one block step of K9 on the list in e->d_hblist: predict every body to t_next, sweep, correct the n_active listed bodies
static int block_step(nbx_engine* e, const nbx::HermiteLevels& lv, int t_next, int n_active)
{
    int stride = 0;
    {
        ProfScope ps(e, NBX_K_INTEGRATE);
        HIP_TRY(nbx::launch_block_predict(e->d_posm, e->d_vel, e->d_hkept, e->d_hbt, e->n, e->n_pad, t_next, lv, e->d_hsrc, e->stream));
    }
    const int rc = block_sweep(e, n_active, &stride);
    if (rc != NBX_OK) return rc;
    {
        ProfScope ps(e, NBX_K_INTEGRATE);
        HIP_TRY(nbx::launch_block_correct(e->d_posm, e->d_vel, e->d_hkept, e->d_hbt, e->d_hblist, n_active, e->d_hpart, e->last.jsplit,
                                          stride, t_next, lv, e->stream));
    }
    e->hblock_steps++;
    e->hblock_evals += n_active;
    return NBX_OK;
}

// G of K10's sweep and room for its partials
static int train_groups(nbx_engine* e, int* groups)
{
    *groups = nbx::hermite_train_groups(e->n_pad / kTile, e->cu_count, e->jsplit);
    return grow(&e->d_hpart, &e->hpart_cap, (size_t)*groups * (size_t)nbx::kTrainMaxBlock);
}

// A macro-step with NBX_OPT_HERMITE_BLOCK_TRAIN = L > 0 (hermite_train.hip).  The scheduler once; then trains of L cars -- a car is
// a block step of at most kTrainMaxBlock bodies, sweep + finish, that finds its block in device memory and leaves the next one
// there -- with ONE read of head + train record behind each train.  A car that meets a larger block (or the end of the macro-step)
// does nothing, and so do the cars behind it: the host then runs K9's block step on the list that is already there, schedules
// again and goes on with trains.
static int train_macro_step(nbx_engine* e, const nbx::HermiteLevels& lv)
{
    const int n = e->n, dim = hermite_sweep_dim(e);
    int groups = 0;
    int rc = train_groups(e, &groups);
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_htrain, &e->htrain_cap, 1);
    if (rc != NBX_OK) return rc;
    if (!e->h_htrain) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->h_htrain), sizeof(*e->h_htrain)));
    nbx::HermiteHead* d_head = reinterpret_cast<nbx::HermiteHead*>(e->d_hbws);
    int large_steps = 0;          // block steps K9 served
    long long large_evals = 0;
    bool schedule = true;
    for (int t_done = 0; t_done < nbx::kHermiteTicks;) {
        if (schedule) {
            ProfScope ps(e, NBX_K_INTEGRATE);
            HIP_TRY(nbx::launch_block_schedule(e->d_hbt, n, e->d_hbws, e->d_hblist, e->stream));
            if (t_done == 0) HIP_TRY(nbx::launch_train_reset(e->d_htrain, e->stream));
            schedule = false;
        }
        for (int car = 0; car < e->hblock_train; car++) {
            {
                ProfScope ps(e, NBX_K_FORCE);
                HIP_TRY(nbx::launch_train_sweep(e->d_posm, e->d_vel, e->d_hkept, e->d_hbt, n, e->n_pad / kTile, groups, dim, d_head, e->d_htrain,
                                                e->d_hblist, 0, lv, e->d_hpart, e->stream, &e->last));
            }
            ProfScope ps(e, NBX_K_INTEGRATE);
            HIP_TRY(nbx::launch_train_finish(e->d_posm, e->d_vel, e->d_hkept, e->d_hbt, n, e->d_hblist, d_head, e->d_htrain, e->d_hpart, groups,
                                             lv, e->stream));
        }
        HIP_TRY(hipMemcpyAsync(&e->h_htrain->head, d_head, sizeof(nbx::HermiteHead), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(&e->h_htrain->train, e->d_htrain, sizeof(nbx::HermiteTrain), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(wait_stream(e->stream, n <= kSpinMaxBodies));
        e->hblock_reads++;
        const nbx::HermiteTrain tr = e->h_htrain->train;
        if (tr.steps < e->hblock_train_steps || tr.steps > e->hblock_train_steps + e->hblock_train)
            return fail(NBX_ERR_STATE, "the block train reports %d steps after %d in a train of %d", tr.steps, e->hblock_train_steps, e->hblock_train);
        if (tr.steps > e->hblock_train_steps) t_done = tr.t_done;
        e->hblock_train_steps = tr.steps;
        e->hblock_steps = large_steps + tr.steps;
        e->hblock_evals = large_evals + tr.evals;
        if (tr.finished || t_done >= nbx::kHermiteTicks) break;
        const int t_next = e->h_htrain->head.t_next, n_active = e->h_htrain->head.n_active;
        if (t_next <= t_done || t_next > nbx::kHermiteTicks || n_active < 1 || n_active > n)
            return fail(NBX_ERR_STATE, "the block scheduler returned t_next = %d after %d with %d of %d bodies", t_next, t_done, n_active, n);
        if (n_active <= nbx::kTrainMaxBlock) continue;   // the train ran out of cars: the next one
        rc = block_step(e, lv, t_next, n_active);
        if (rc != NBX_OK) return rc;
        large_steps++;
        large_evals += n_active;
        t_done = t_next;
        schedule = true;
    }
    return NBX_OK;
}

static bool block_usable(const nbx_engine* e) { return hermite_kept_usable(e) && e->hblock_valid && e->d_hbt; }

int step_hermite_block(nbx_engine* e, float dt_max, float eta)
{
    int rc = hermite_ready(e);   // (an upload of new host state takes the kept pair, and the levels with it: positions_moved())
    if (rc != NBX_OK) return rc;
    if (!(dt_max > 0.0f) || !std::isfinite(dt_max)) return fail(NBX_ERR_INVALID, "dt_max must be positive and finite");
    e->hblock_steps = 0;
    e->hblock_evals = 0;
    e->hblock_train_steps = 0;
    e->hblock_reads = 0;
    const int n = e->n;
    if (n == 0) return NBX_OK;
    if (!hermite_kept_usable(e)) {
        rc = hermite_evaluate_kept(e);
        if (rc != NBX_OK) return rc;
    }
    rc = block_buffers(e);
    if (rc != NBX_OK) return rc;
    const nbx::HermiteLevels lv = nbx::hermite_levels(dt_max, eta > 0.0f ? eta : 0.0f);
    if (!(block_usable(e) && (e->hblock_any_dt || e->hblock_dt_max == dt_max))) {
        ProfScope ps(e, NBX_K_INTEGRATE);
        HIP_TRY(nbx::launch_block_init_levels(e->d_hkept, n, lv, e->d_hbt, e->stream));
    }
    e->hermite_valid = false;   // until the last corrector is enqueued
    e->hblock_valid = false;
    const int dim = hermite_sweep_dim(e);
    if (e->hblock_train > 0) {
        rc = train_macro_step(e, lv);
        if (rc != NBX_OK) return rc;
    } else {
        for (int t_done = 0; t_done < nbx::kHermiteTicks;) {
            {
                ProfScope ps(e, NBX_K_INTEGRATE);
                HIP_TRY(nbx::launch_block_schedule(e->d_hbt, n, e->d_hbws, e->d_hblist, e->stream));
            }
            HIP_TRY(hipMemcpyAsync(e->h_hbhead, e->d_hbws, sizeof(nbx::HermiteHead), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(wait_stream(e->stream, n <= kSpinMaxBodies));
            e->hblock_reads++;
            const int t_next = e->h_hbhead->t_next, n_active = e->h_hbhead->n_active;
            if (t_next <= t_done || t_next > nbx::kHermiteTicks || n_active < 1 || n_active > n)
                return fail(NBX_ERR_STATE, "the block scheduler returned t_next = %d after %d with %d of %d bodies", t_next, t_done, n_active, n);
            rc = block_step(e, lv, t_next, n_active);
            if (rc != NBX_OK) return rc;
            t_done = t_next;
        }
    }
    e->positions_moved();       // (the order-sorted copy of the positions is stale from here) ...
    e->hermite_valid = true;    // ... but kept pair and levels are the ones this macro-step left
    e->hermite_dim = dim;
    e->hblock_valid = true;
    e->hblock_any_dt = false;
    e->hblock_dt_max = dt_max;
    e->host_pos_valid = false;
    e->host_vel_valid = false;
    if (log_enabled())
        std::fprintf(stderr, "[nbx] step_hermite_block dev=%d n=%d dt_max=%g eta=%g block steps=%d evaluations=%lld (last: S=%d T=%d)\n",
                     e->device, n, (double)dt_max, (double)eta, e->hblock_steps, e->hblock_evals, e->last.jsplit, e->last.bpt);
    return NBX_OK;
}

int hermite_block_set_levels(nbx_engine* e, const int32_t* levels, int n)
{
    int rc = hermite_ready(e);
    if (rc != NBX_OK) return rc;
    if (!levels || n != e->n) return fail(NBX_ERR_INVALID, "%d levels for %d particles", levels ? n : 0, e->n);
    std::vector<nbx::HermiteBody> bt((size_t)n);
    for (int i = 0; i < n; i++) {
        if (levels[i] < 0 || levels[i] > nbx::kHermiteMaxLevel)
            return fail(NBX_ERR_INVALID, "level %d of body %d is outside 0 .. %d", levels[i], i, nbx::kHermiteMaxLevel);
        bt[(size_t)i] = nbx::HermiteBody{0, levels[i]};
    }
    if (n == 0) return NBX_OK;
    if (!hermite_kept_usable(e)) {
        rc = hermite_evaluate_kept(e);
        if (rc != NBX_OK) return rc;
    }
    rc = block_buffers(e);
    if (rc != NBX_OK) return rc;
    e->hblock_valid = false;
    HIP_TRY(hipMemcpyAsync(e->d_hbt, bt.data(), sizeof(nbx::HermiteBody) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));   // (bt is pageable and leaves scope)
    e->hblock_valid = true;
    e->hblock_any_dt = true;
    return NBX_OK;
}

int hermite_block_levels(nbx_engine* e, int cap, int32_t* out)
{
    int rc = hermite_ready(e);
    if (rc != NBX_OK) return rc;
    const int n = e->n;
    if (cap < n || !out) return fail(NBX_ERR_INVALID, "capacity %d < particle count %d", out ? cap : 0, n);
    if (n == 0) return 0;
    if (!block_usable(e)) return fail(NBX_ERR_STATE, "no block levels: nothing has set them since the state last changed");
    std::vector<nbx::HermiteBody> bt((size_t)n);
    HIP_TRY(hipMemcpyAsync(bt.data(), e->d_hbt, sizeof(nbx::HermiteBody) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < n; i++) out[i] = bt[(size_t)i].level;
    return n;
}

static int download_aj(nbx_engine* e, const nbx::HermiteAJ* d, int count, float* ax, float* ay, float* az, float* jx, float* jy, float* jz)
{
    std::vector<nbx::HermiteAJ> tmp((size_t)count);
    HIP_TRY(hipMemcpyAsync(tmp.data(), d, sizeof(nbx::HermiteAJ) * (size_t)count, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < count; i++) {
        if (ax) ax[i] = tmp[i].a.x;
        if (ay) ay[i] = tmp[i].a.y;
        if (az) az[i] = tmp[i].a.z;
        if (jx) jx[i] = tmp[i].j.x;
        if (jy) jy[i] = tmp[i].j.y;
        if (jz) jz[i] = tmp[i].j.z;
    }
    return count;
}

int hermite_kept(nbx_engine* e, int cap, float* ax, float* ay, float* az, float* jx, float* jy, float* jz)
{
    int rc = hermite_ready(e);
    if (rc != NBX_OK) return rc;
    if (cap < e->n) return fail(NBX_ERR_INVALID, "capacity %d < particle count %d", cap, e->n);
    if (e->n == 0) return 0;
    if (!hermite_kept_usable(e)) return fail(NBX_ERR_STATE, "no kept (a0, j0): the state changed since the last Hermite step or nbx_acc_jerk");
    return download_aj(e, e->d_hkept, e->n, ax, ay, az, jx, jy, jz);
}

int acc_jerk_subset(nbx_engine* e, const int32_t* idx, int count, float* ax, float* ay, float* az, float* jx, float* jy, float* jz)
{
    int rc = hermite_ready(e);
    if (rc != NBX_OK) return rc;
    if (count < 0 || (count > 0 && !idx)) return fail(NBX_ERR_INVALID, "bad index list (count %d)", count);
    for (int k = 0; k < count; k++)
        if (idx[k] < 0 || idx[k] >= e->n) return fail(NBX_ERR_INVALID, "index %d (entry %d) is outside 0 .. %d", idx[k], k, e->n - 1);
    if (count == 0) return 0;
    rc = grow(&e->d_hsrc, &e->hsrc_cap, (size_t)e->n_pad);
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_hblist, &e->hblist_cap, (size_t)std::max(count, e->n));
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_hbout, &e->hbout_cap, (size_t)count);
    if (rc != NBX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_hblist, idx, sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, e->stream));
    if (e->hblock_train > 0 && count <= nbx::kTrainMaxBlock) {   // K10's sweep reads posm / vel itself: no source records
        int groups = 0;
        rc = train_groups(e, &groups);
        if (rc != NBX_OK) return rc;
        {
            ProfScope ps(e, NBX_K_FORCE);
            HIP_TRY(nbx::launch_train_sweep(e->d_posm, e->d_vel, nullptr, nullptr, e->n, e->n_pad / kTile, groups, hermite_sweep_dim(e), nullptr,
                                            nullptr, e->d_hblist, count, nbx::HermiteLevels{}, e->d_hpart, e->stream, &e->last));
        }
        HIP_TRY(nbx::launch_block_keep(count, e->d_hpart, groups, nbx::kTrainMaxBlock, e->d_hbout, e->stream));
        return download_aj(e, e->d_hbout, count, ax, ay, az, jx, jy, jz);
    }
    {   // the bodies as they are: the kept pair is neither read nor written
        ProfScope ps(e, NBX_K_INTEGRATE);
        HIP_TRY(nbx::launch_hermite_predict(e->d_posm, e->d_vel, nullptr, e->n, e->n_pad, false, 0.0f, e->d_hsrc, e->stream));
    }
    int stride = 0;
    rc = block_sweep(e, count, &stride);
    if (rc != NBX_OK) return rc;
    HIP_TRY(nbx::launch_block_keep(count, e->d_hpart, e->last.jsplit, stride, e->d_hbout, e->stream));
    return download_aj(e, e->d_hbout, count, ax, ay, az, jx, jy, jz);   // (its synchronise also covers the pageable index list)
}

}  // namespace nbxi
