// engine_acc_jerk64.cpp -- host side of K12 (acc_jerk64.hip): nbx_acc_jerk_f64.  Reads the live device state (posm, vel) and writes
// workspaces of its own -- records, partials, list, output -- so nothing the stepping paths use is touched: not the kept (a0, j0) of
// the Hermite family, not its validity flags, levels or train record.  An integrator that calls it between two steps continues bit
// for bit as if it had not.  It does not go through hermite_ready (that one refuses the Newtonian law; this sweep serves it).
#include "engine_internal.h"

namespace nbxi {

// T of the sweep: NBX_ACC_JERK64_T = 1 | 2 | 4 (the A/B of docs/rounds/r13.md), else NBX_OPT_BODIES_PER_THREAD (2 or 4) when it is set,
// else acc_jerk64_targets
static int sweep_targets(const nbx_engine* e, int count)
{
    static const int forced = [] {
        const char* s = std::getenv("NBX_ACC_JERK64_T");
        const int t = s ? std::atoi(s) : 0;
        return t == 1 || t == 2 || t == 4 ? t : 0;
    }();
    return forced ? forced : e->bpt > 0 ? e->bpt : nbx::acc_jerk64_targets(count);
}

int acc_jerk_f64(nbx_engine* e, const int32_t* idx, int count, double* ax, double* ay, double* az, double* jx, double* jy, double* jz)
{
    int rc = ensure_device(e);
    if (rc != NBX_OK) return rc;
    if (e->world > 1) return fail(NBX_ERR_STATE, "the fp64 acceleration + jerk sweep serves unsharded engines: the other slabs' velocities are not on this rank");
    if (e->in_group) return fail(NBX_ERR_STATE, "the fp64 acceleration + jerk sweep serves single engines, not members of an nbx_group");
    rc = newton_refusal(e);
    if (rc != NBX_OK) return rc;
    rc = upload(e);   // (resolves a Barnes-Hut step still in flight)
    if (rc != NBX_OK) return rc;
    const int n = e->n;
    if (count < 0) return fail(NBX_ERR_INVALID, "bad count %d", count);
    if (!idx && count < n) return fail(NBX_ERR_INVALID, "capacity %d < particle count %d", count, n);
    for (int k = 0; idx && k < count; k++)
        if (idx[k] < 0 || idx[k] >= n) return fail(NBX_ERR_INVALID, "index %d (entry %d) is outside 0 .. %d", idx[k], k, n - 1);
    const int targets = idx ? count : n;
    if (n == 0 || targets == 0) return 0;
    const int t = sweep_targets(e, targets);
    const int split = nbx::acc_jerk64_split(targets, n, e->cu_count, t, e->jsplit);
    const int stride = nbx::acc_jerk64_stride(targets, t);
    rc = grow(&e->d_aj64src, &e->aj64src_cap, (size_t)n);
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_aj64part, &e->aj64part_cap, (size_t)split * (size_t)stride);
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_aj64out, &e->aj64out_cap, (size_t)targets);
    if (rc != NBX_OK) return rc;
    if (idx) {
        rc = grow(&e->d_aj64list, &e->aj64list_cap, (size_t)count);
        if (rc != NBX_OK) return rc;
        HIP_TRY(hipMemcpyAsync(e->d_aj64list, idx, sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, e->stream));
    }
    {
        ProfScope ps(e, NBX_K_FORCE);
        HIP_TRY(nbx::launch_widen_aj64(e->d_posm, e->d_vel, e->d_aj64src, n, e->stream));
        HIP_TRY(nbx::launch_acc_jerk64(e->d_aj64src, idx ? e->d_aj64list : nullptr, targets, n, e->law, split, t, e->d_aj64part, e->stream,
                                       &e->last));
        HIP_TRY(nbx::launch_reduce_aj64(targets, e->d_aj64part, split, stride, e->d_aj64out, e->stream));
    }
    std::vector<nbx::AccJerk64> tmp((size_t)targets);
    HIP_TRY(hipMemcpyAsync(tmp.data(), e->d_aj64out, sizeof(nbx::AccJerk64) * (size_t)targets, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));   // (also covers the pageable index list)
    for (int i = 0; i < targets; i++) {
        if (ax) ax[i] = tmp[i].a.x;
        if (ay) ay[i] = tmp[i].a.y;
        if (az) az[i] = tmp[i].a.z;
        if (jx) jx[i] = tmp[i].j.x;
        if (jy) jy[i] = tmp[i].j.y;
        if (jz) jz[i] = tmp[i].j.z;
    }
    if (log_enabled())
        std::fprintf(stderr, "[nbx] acc_jerk_f64 dev=%d n=%d targets=%d law=%d S=%d T=%d\n", e->device, n, targets, e->law, split, t);
    return targets;
}

}  // namespace nbxi
