// hermite_block_math.h -- the device arithmetic that hermite_block.hip (K9) and hermite_train.hip (K10) must perform in ONE order:
// the prediction of a body over its own span, and the corrector with the level rule.  Same operations, same order, every product
// and sum rounded on its own: a body predicted by either unit has the same bits, and a block step gives the same state whichever
// unit served it up to the order of the pair sums.
#pragma once
#include "hermite_math.h"

namespace nbx {

__device__ __forceinline__ int step_of(const int level) { return kHermiteTicks >> level; }

// body (p, v, kept pair k) standing at b.t, advanced to t_next with k_hermite_predict's formula in its order.  A span that is the
// body's own step takes the host-rounded (dt, c2, c3) of its level; any other span dt = float(span) tick, c2 = (0.5 dt) dt,
// c3 = (c2 dt) (1/3)
__device__ __forceinline__ HermiteSrc block_predict_body(const float4 p, const float4 v, const HermiteAJ& k, const HermiteBody b,
                                                         const int t_next, const HermiteLevels& lv)
{
    const int span = t_next - b.t;
    float dt, c2, c3;
    if (span == step_of(b.level)) {
        dt = lv.dt[b.level]; c2 = lv.c2[b.level]; c3 = lv.c3[b.level];
    } else {
        dt = __fmul_rn((float)span, lv.tick);
        c2 = __fmul_rn(__fmul_rn(0.5f, dt), dt);
        c3 = __fmul_rn(__fmul_rn(c2, dt), 1.0f / 3.0f);
    }
    HermiteSrc r{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    r.m = p.w;
    r.x = __fadd_rn(__fadd_rn(__fadd_rn(p.x, __fmul_rn(dt, v.x)), __fmul_rn(c2, k.a.x)), __fmul_rn(c3, k.j.x));
    r.y = __fadd_rn(__fadd_rn(__fadd_rn(p.y, __fmul_rn(dt, v.y)), __fmul_rn(c2, k.a.y)), __fmul_rn(c3, k.j.y));
    r.z = __fadd_rn(__fadd_rn(__fadd_rn(p.z, __fmul_rn(dt, v.z)), __fmul_rn(c2, k.a.z)), __fmul_rn(c3, k.j.z));
    r.vx = __fadd_rn(__fadd_rn(v.x, __fmul_rn(dt, k.a.x)), __fmul_rn(c2, k.j.x));
    r.vy = __fadd_rn(__fadd_rn(v.y, __fmul_rn(dt, k.a.y)), __fmul_rn(c2, k.j.y));
    r.vz = __fadd_rn(__fadd_rn(v.z, __fmul_rn(dt, k.a.z)), __fmul_rn(c2, k.j.z));
    return r;
}

// the corrector on body i with its new (a1, j1) = n1, scattered to posm / vel / kept; t_i = t_next (0 at the end of the
// macro-step); then, unless levels are frozen, the new level from dt_req = eta |a1| / |j1|: deeper while dt(level) > dt_req, else
// one level up if 2 dt(level) <= dt_req and t_next is a multiple of the doubled step
__device__ __forceinline__ void block_correct_body(float4* __restrict__ posm, float4* __restrict__ vel, HermiteAJ* __restrict__ kept,
                                                   HermiteBody* __restrict__ bt, const int i, const HermiteAJ& n1, const int t_next,
                                                   const HermiteLevels& lv)
{
    const HermiteAJ n0 = kept[i];
    int level = bt[i].level;
    const float h = lv.h[level], c12 = lv.c12[level];
    float4 v = vel[i];
    float4 p = posm[i];
    const float v1x = correct_v(v.x, n0.a.x, n1.a.x, n0.j.x, n1.j.x, h, c12);
    const float v1y = correct_v(v.y, n0.a.y, n1.a.y, n0.j.y, n1.j.y, h, c12);
    const float v1z = correct_v(v.z, n0.a.z, n1.a.z, n0.j.z, n1.j.z, h, c12);
    p.x = correct_x(p.x, v.x, v1x, n0.a.x, n1.a.x, h, c12);
    p.y = correct_x(p.y, v.y, v1y, n0.a.y, n1.a.y, h, c12);
    p.z = correct_x(p.z, v.z, v1z, n0.a.z, n1.a.z, h, c12);
    v.x = v1x; v.y = v1y; v.z = v1z;
    posm[i] = p;
    vel[i] = v;
    kept[i] = n1;
    if (lv.eta > 0.f) {
        const float dt_req = __fmul_rn(lv.eta, hermite_ratio(n1));
        if (lv.dt[level] > dt_req && level < kHermiteMaxLevel) {
            do level++; while (lv.dt[level] > dt_req && level < kHermiteMaxLevel);
        } else if (level > 0 && lv.dt[level - 1] <= dt_req && (t_next & (2 * step_of(level) - 1)) == 0) {
            level--;
        }
    }
    bt[i] = HermiteBody{t_next == kHermiteTicks ? 0 : t_next, level};
}

}  // namespace nbx
