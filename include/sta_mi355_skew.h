/*
 * sta_mi355_skew.h - included by sta_mi355_debug.h under -DSTA_WAVE_SKEW and by nothing else.
 */
#ifndef STA_MI355_SKEW_H
#define STA_MI355_SKEW_H
#include "sta_mi355.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Wave-skew schedule tests (csrc/sta_skew.h, tests/test_skew_gpu.py): the two entry points that libsta_mi355_skew.so ALONE exports, the third build of the main
 * translation unit (-DSTA_TEST_HOOKS -DSTA_WAVE_SKEW), whose kernels carry a skew point behind every barrier, at kernel entry and in
 * front of every epilogue.  sta_debug_set_wave_skew: bit w of wave_mask (16 bits) delays wave w of every workgroup at every point
 * whose bit (id & 63) is set in point_hi:point_lo, by repeat x s_sleep 127; bit 16 of wave_mask measures the intervals between the
 * points of every wave instead and delays nothing.  Resets the counters.  sta_debug_wave_skew_hits: out[34]; out[0] = points hit by selected
 * waves since then, out[1] = the largest measured interval in 10-ns ticks, out[2 .. 33] = bit id set when point id (< 2048) was hit.  Both synchronise the device; the configuration is a
 * __device__ variable of that library. */
STA_API int sta_debug_set_wave_skew(unsigned wave_mask, unsigned point_lo, unsigned point_hi, unsigned repeat);
STA_API int sta_debug_wave_skew_hits(unsigned long long* out);

#ifdef __cplusplus
}
#endif
#endif
