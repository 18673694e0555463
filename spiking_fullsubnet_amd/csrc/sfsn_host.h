// Host-only helpers of the launch layer, shared by every .hip unit that launches: status mapping, per-device caches, the launch
// with raised dynamic LDS, the checks and the copy of a sfsn_scan_segment, and the tuning knobs of experiment builds.
// Nothing here reaches the device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "sfsn.h"

static inline int hip_ok(hipError_t e) { return e == hipSuccess ? SFSN_OK : SFSN_EHIP; }
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Per-DEVICE caches: one process may drive several GPUs (the function attribute below and the CU count are per device).
#define SFSN_MAX_DEVICES 64
static inline int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SFSN_MAX_DEVICES) dev = 0;
    return dev;
}
static inline int cu_count() {  // compute units of the current device (256 on MI355X); 256 if the query fails
    static int n[SFSN_MAX_DEVICES] = {0};
    const int dev = current_device();
    if (n[dev] == 0) {
        int v = 0;
        n[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    }
    return n[dev];
}
// hipFuncAttributeMaxDynamicSharedMemorySize raised to `bytes` on the current device (idempotent; a benign race between host
// threads sets it twice at worst).  `seen` is the caller's per-kernel table of the largest size set per device.
static inline int raise_lds(const void* kern, int bytes, int* seen) {
    const int dev = current_device();
    if (bytes > seen[dev]) {
        if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return SFSN_EHIP;
        seen[dev] = bytes;
    }
    return SFSN_OK;
}
// Kernel `Kern` may be launched with `lds` bytes of dynamic LDS: above the 64 KiB every kernel may have, its limit is raised (once
// per kernel, device and size: the table is this instantiation's own; not a stream operation).
template <auto Kern>
static int allow_lds(size_t lds) {
    static int seen[SFSN_MAX_DEVICES] = {0};
    return lds > 64 * 1024 ? raise_lds(reinterpret_cast<const void*>(Kern), (int)lds, seen) : SFSN_OK;
}
// One launch of kernel `Kern` with `lds` bytes of dynamic LDS.
template <auto Kern, class... Args>
static int launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args) {
    if (allow_lds<Kern>(lds) != SFSN_OK) return SFSN_EHIP;
    hipLaunchKernelGGL(Kern, grid, block, lds, st, args...);
    return hip_ok(hipGetLastError());
}

// ---- sfsn_scan_segment: what every scan / stack entry point asks of a segment, and what it hands to the device as it is
enum {
    SEG_NEED_ZIN = 1,     // the precomputed input term is required
    SEG_NO_ZIN = 2,       // the launch forms the input term itself: `zin` is ignored (neither checked nor passed on)
    SEG_MEMBRANE = 4,     // a membrane output is allowed (the per-layer scans; needs the fp32 spikes, `out` bit 2)
    SEG_DEFER_ALIGN = 8,  // the caller calls segment_aligned itself, behind checks of its own that answer first
};
static inline bool segment_aligned(const sfsn_scan_segment& s, int flags) {
    return ((flags & SEG_NO_ZIN) || aligned16(s.zin)) && aligned16(s.w_hh) && aligned16(s.h_state) && aligned16(s.c_state) &&
           aligned16(s.spikes_f32) && aligned16(s.spikes_i8) && aligned16(s.membrane);
}
// `out`: the launch's output set (bit 0 fp32 spikes, bit 2 membranes), the same for every segment -- it selects the kernel variant;
// the int8 spikes are always produced (every consumer of a scan in this library reads them)
static inline int check_segment(const sfsn_scan_segment& s, int out, int flags) {
    if (!s.spikes_i8 || (s.spikes_f32 != nullptr) != ((out & 1) != 0)) return SFSN_EINVAL;
    if ((flags & SEG_MEMBRANE) ? (s.membrane != nullptr) != ((out & 4) != 0) : s.membrane != nullptr) return SFSN_EINVAL;
    if (s.R <= 0 || !s.w_hh || !s.w_dq || !s.bias || !s.bn_alpha || !s.bn_beta || !s.h_state || !s.c_state) return SFSN_EINVAL;
    if ((flags & SEG_NEED_ZIN) && !s.zin) return SFSN_EINVAL;
    if (!(flags & SEG_DEFER_ALIGN) && !segment_aligned(s, flags)) return SFSN_EINVAL;
    return SFSN_OK;
}
// Dev: ScanSegDev, or a role of the stack launch (the fields of the same names)
template <class Dev>
static inline void copy_segment(Dev& d, const sfsn_scan_segment& s, int flags) {
    d.zin = (flags & SEG_NO_ZIN) ? nullptr : const_cast<float*>(s.zin);
    d.w_hh = s.w_hh; d.w_dq = s.w_dq; d.bias = s.bias; d.bn_alpha = s.bn_alpha; d.bn_beta = s.bn_beta;
    d.h_state = s.h_state; d.c_state = s.c_state; d.spikes_f32 = s.spikes_f32; d.spikes_i8 = s.spikes_i8; d.count = s.spike_count;
    d.R = s.R;
}

// ---- tuning knobs of A/B runs: the product library reads none of them (a stray environment variable cannot change a launch);
//      a build with -DSFSN_TIMING_EXPERIMENTS (scripts/build_exp_lib.sh) reads the environment variable of the same name
#ifdef SFSN_TIMING_EXPERIMENTS
static inline int sfsn_knob(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
static inline bool sfsn_knob_set(const char* name) { return getenv(name) != nullptr; }
#else
static inline int sfsn_knob(const char*, int dflt) { return dflt; }
static inline bool sfsn_knob_set(const char*) { return false; }
#endif
static inline int sfsn_knob(const char* name, int dflt, int lo, int hi) {
    const int x = sfsn_knob(name, dflt);
    return x < lo ? lo : (x > hi ? hi : x);
}
#ifdef SFSN_S3_LSPLIT  // (units that include sfsn_scan3_dev.h before this header: the built-in defaults are its macros)
// fp32 store instructions per frame the loader wave of the 8-row IO-wave scans takes, and the FUSEDX3 role's own value
static inline int s3_lsplit_knob() { return sfsn_knob("SFSN_S3_LSPLIT", SFSN_S3_LSPLIT, 0, 16); }
static inline int s3x_lsplit_knob() { return sfsn_knob("SFSN_S3X_LSPLIT", SFSN_S3X_LSPLIT, 0, 16); }
#endif
