// engine_diag.cpp -- host side of K7 and its Newtonian sibling (diag64.hip): nbx_forces_f64 and nbx_conserved.  Both read the live device state (posm, the
// slab's velocities) and write workspaces of their own; nothing the stepping paths use is touched.
#include "engine_internal.h"

namespace nbxi {

// widen, sweep, reduce: leaves (Fx, Fy, Fz, phi) of the slab's targets in e->d_out64 (enqueued, not waited for)
static int sweep_f64(nbx_engine* e, bool pot)
{
    const int slab = e->slab(), n = e->n;
    const int split = nbx::sweep64_split(slab, n, e->cu_count);
    const int stride = nbx::sweep64_stride(slab);
    int rc = grow(&e->d_src64, &e->src64_cap, (size_t)n);
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_part64, &e->part64_cap, (size_t)split * (size_t)stride);
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_out64, &e->out64_cap, (size_t)slab);
    if (rc != NBX_OK) return rc;
    HIP_TRY(nbx::launch_widen64(e->d_posm, e->d_src64, n, e->stream));
    if (e->law == 1) {   // the Newtonian law: phi_i = -sum m_j / sqrt(s) needs no 1/2 (k_conserved64's 1/2 m_i phi_i is the pair energy)
        HIP_TRY(nbx::launch_newton64(e->d_posm, e->d_src64, e->lo, slab, n, split, pot, e->d_part64, e->stream, &e->last));
        HIP_TRY(nbx::launch_reduce64(e->d_posm, e->lo, slab, e->d_part64, split, e->d_out64, e->stream, 1.0));
        return NBX_OK;
    }
    HIP_TRY(nbx::launch_sweep64(e->d_posm, e->d_src64, e->lo, slab, n, split, pot, e->d_part64, e->stream, &e->last));
    HIP_TRY(nbx::launch_reduce64(e->d_posm, e->lo, slab, e->d_part64, split, e->d_out64, e->stream));
    return NBX_OK;
}

// what both entry points check first; the upload resolves a Barnes-Hut step still in flight (ensure_device)
static int diag_ready(nbx_engine* e)
{
    if (e->in_group) return fail(NBX_ERR_STATE, "the fp64 sweep serves single engines, not members of an nbx_group");
    const int nrc = newton_refusal(e);
    if (nrc != NBX_OK) return nrc;
    return upload(e);
}

int forces_f64(nbx_engine* e, int cap, double* fx, double* fy, double* fz, double* phi)
{
    int rc = diag_ready(e);
    if (rc != NBX_OK) return rc;
    const int slab = e->slab();
    if (cap < slab) return fail(NBX_ERR_INVALID, "capacity %d < slab %d", cap, slab);
    if (slab == 0) return 0;
    rc = sweep_f64(e, phi != nullptr);
    if (rc != NBX_OK) return rc;
    std::vector<double4> tmp((size_t)slab);
    HIP_TRY(hipMemcpyAsync(tmp.data(), e->d_out64, sizeof(double4) * (size_t)slab, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < slab; i++) {
        if (fx) fx[i] = tmp[i].x;
        if (fy) fy[i] = tmp[i].y;
        if (fz) fz[i] = tmp[i].z;
        if (phi) phi[i] = tmp[i].w;
    }
    return slab;
}

int conserved_f64(nbx_engine* e, int count, double* out)
{
    int rc = diag_ready(e);
    if (rc != NBX_OK) return rc;
    if (count != NBX_CONS_COUNT || !out) return fail(NBX_ERR_INVALID, "count must be NBX_CONS_COUNT (%d) and out non-null", (int)NBX_CONS_COUNT);
    const int slab = e->slab();
    for (int k = 0; k < NBX_CONS_COUNT; k++) out[k] = 0.0;
    if (slab == 0) return NBX_OK;
    rc = sweep_f64(e, true);
    if (rc != NBX_OK) return rc;
    rc = grow(&e->d_cons64, &e->cons64_cap, (size_t)NBX_CONS_COUNT + nbx::conserved64_workspace(slab));
    if (rc != NBX_OK) return rc;
    HIP_TRY(nbx::launch_conserved64(e->d_posm, e->lo, slab, e->d_vel, e->d_out64, e->d_cons64 + NBX_CONS_COUNT, e->d_cons64, e->stream));
    HIP_TRY(hipMemcpyAsync(out, e->d_cons64, sizeof(double) * NBX_CONS_COUNT, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return NBX_OK;
}

}  // namespace nbxi
