// Skew points: the schedule tests of tests/test_skew_gpu.py delay chosen waves of a workgroup right behind every barrier, at kernel
// entry and in front of every epilogue, and demand the same exact results.  A kernel that hands data between waves through LDS (or
// through global memory behind a workgroup barrier) with a missing or misplaced barrier then fails every time instead of once in many
// processes.
//
//   STA_SKEW(id)        directly behind a __syncthreads() / raw s_barrier statement
//   STA_SKEW_ENTRY(id)  first statement of a kernel with more than one wave per workgroup that has a barrier
//   STA_SKEW_EPI(id)    in front of an epilogue that reuses LDS
//
// Without -DSTA_WAVE_SKEW (the product, the test-hooks library, every handle-free library) the three expand to NOTHING: those
// libraries' device code is what it is without this header.  With it (libsta_mi355_skew.so alone) a point reads the configuration
// below; when bit `wave index in the workgroup` of wave_mask and bit `id & 63` of the point mask are both set, the wave counts one
// hit from one lane and sleeps repeat x s_sleep 127 (127 x 64 clocks: 3.4 us at 2.4 GHz, longer at a lower clock).  The condition
// is built from readfirstlane values and configuration words: wave-uniform, no divergence inside the wave.  No barrier, no LDS.
//
// The counted waits of the ring main loop (gemm2.h: s_waitcnt vmcnt(n) + s_barrier) count vector memory instructions in flight, and
// the hit is one: a delayed wave drains its own counter (vmcnt(0)) before it goes on, so that the count in front of the next
// barrier means what it means in the product - never fewer loads landed than there, only more, and only in the wave that has just
// slept for microseconds anyway.  Waves that are not selected execute two scalar loads and a branch.
//
// Bit 16 of wave_mask: measure instead of delay (profiles/r33_wave_skew.txt).  Every point of every wave then notes the 100 MHz
// clock per (workgroup, wave), counts no hit and keeps the largest distance between two consecutive points of one wave of one
// launch - the longest barrier-to-barrier interval, waiting time at the barrier included - the figure the tests' repeat counts are
// derived from.
#pragma once
#ifdef STA_WAVE_SKEW
#include <hip/hip_runtime.h>
#define STA_SKEW_IDS 2048                   // point ids are below this
struct StaSkewCfg {
    unsigned wave_mask, point_lo, point_hi, repeat;
    unsigned long long hits, max_gap;       // max_gap in ticks of the 100 MHz clock
    unsigned seen[STA_SKEW_IDS / 32];       // bit id: point id was hit by a selected wave (which kernel, which site - not only how often)
};
__device__ StaSkewCfg g_sta_skew;
#define STA_SKEW_SLOTS 65536                // (workgroup over x, y and z; wave) slots of the measuring mode; grids beyond 4096 workgroups wrap (a wrapped slot can only shorten a gap, or
__device__ unsigned long long g_sta_skew_last[STA_SKEW_SLOTS];      //  lengthen it by the other workgroup's lifetime: measure on grids that fit)

__device__ __forceinline__ void sta_skew_point(const int id, const bool entry) {
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned wmask = g_sta_skew.wave_mask;
    const unsigned pmask = (id & 32) ? g_sta_skew.point_hi : g_sta_skew.point_lo;
    if (wmask & 0x10000u) {
        if (__lane_id() == 0) {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            const unsigned wg = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);      // the workgroup's linear index in its grid
            unsigned long long* slot = g_sta_skew_last + ((wg * 16u + wave) & (STA_SKEW_SLOTS - 1));
            // the slot is this wave's own: a plain load and store, and an atomic on the one shared word only for a new maximum (an
            // atomic per point from every wave of the grid measures its own queue)
            const unsigned long long prev = *slot;
            *slot = now;
            if (!entry && prev != 0 && now > prev && now - prev > g_sta_skew.max_gap) atomicMax(&g_sta_skew.max_gap, now - prev);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }
    if (((wmask >> wave) & 1u) && ((pmask >> (id & 31)) & 1u)) {
        if (__lane_id() == 0) {
            atomicAdd(&g_sta_skew.hits, 1ull);
            if (!((g_sta_skew.seen[(id >> 5) & (STA_SKEW_IDS / 32 - 1)] >> (id & 31)) & 1u)) atomicOr(&g_sta_skew.seen[(id >> 5) & (STA_SKEW_IDS / 32 - 1)], 1u << (id & 31));
        }
        const unsigned rep = g_sta_skew.repeat;
        for (unsigned r = 0; r < rep; ++r) __builtin_amdgcn_s_sleep(127);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}
#define STA_SKEW(id) sta_skew_point(id, false)
#define STA_SKEW_ENTRY(id) sta_skew_point(id, true)
#define STA_SKEW_EPI(id) sta_skew_point(id, false)
#else
#define STA_SKEW(id)
#define STA_SKEW_ENTRY(id)
#define STA_SKEW_EPI(id)
#endif
