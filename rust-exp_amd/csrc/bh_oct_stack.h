// bh_oct_stack.h -- the wave-level stack of the octree walks (bh_oct_walk.hip, bh_oct_newton.hip): opened children wait as
// (record, 64-bit lane mask), last slot first: lanes of three VGPRs, then LDS for the worst case of 7 pending per level x 21
// levels -- the stack cannot overflow.
#pragma once
#include "kernels.h"

namespace nbx {

typedef unsigned long long u64;

constexpr int kOctSpill = 7 * kOctLevels - 64;   // entries beyond the 64 lanes

__device__ __forceinline__ int oct_writelane(const int value, const int lane, int reg)
{
    // (VOP3 takes one SGPR: the lane select goes through m0)
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tv_writelane_b32 %0, %1, m0" : "+v"(reg) : "s"(value), "s"(lane) : "m0");
    return reg;
}

struct OctStack {
    int g = 0, lo = 0, hi = 0;   // lanes = entries
    int sp = 0;                  // wave-uniform
    __device__ __forceinline__ void push(const int group, const u64 mask, volatile int* spill)
    {
        if (sp < 64) {
            g = oct_writelane(group, sp, g);
            lo = oct_writelane((int)(unsigned)mask, sp, lo);
            hi = oct_writelane((int)(unsigned)(mask >> 32), sp, hi);
        } else if (sp - 64 < kOctSpill) {
            if (threadIdx.x == 0) {
                spill[3 * (sp - 64) + 0] = group;
                spill[3 * (sp - 64) + 1] = (int)(unsigned)mask;
                spill[3 * (sp - 64) + 2] = (int)(unsigned)(mask >> 32);
            }
        }
        sp++;
    }
    __device__ __forceinline__ void pop(int& group, u64& mask, volatile int* spill)
    {
        sp--;
        int a, b, c;
        if (sp < 64) {
            a = __builtin_amdgcn_readlane(g, sp);
            b = __builtin_amdgcn_readlane(lo, sp);
            c = __builtin_amdgcn_readlane(hi, sp);
        } else if (sp - 64 < kOctSpill) {
            a = __builtin_amdgcn_readfirstlane(spill[3 * (sp - 64) + 0]);
            b = __builtin_amdgcn_readfirstlane(spill[3 * (sp - 64) + 1]);
            c = __builtin_amdgcn_readfirstlane(spill[3 * (sp - 64) + 2]);
        } else {   // unreachable (see kOctSpill): an empty mask -- the record is loaded and nobody is inside
            a = 0; b = 0; c = 0;
        }
        group = a;
        mask = (u64)(unsigned)b | ((u64)(unsigned)c << 32);
    }
};

}  // namespace nbx
