// sfsn_hop_dev.h -- device helpers of the one-launch streaming hops (sfsn_hop.hip, sfsn_fullband_hop.hip): agent-scope accesses,
// the launch tag and the gather of a data-tagged spike block.  gfx950 only.
#ifndef SFSN_HOP_DEV_H
#define SFSN_HOP_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfsn_scan_dev.h"

#define HOP_THREADS 512
#define HOP_WAVES 8
#define HOP_KS_MAX 5     // 64-wide k steps of the int8 products: H <= 320
#define HOP_SPIN_LIMIT 2000000u

// ---- coherent accesses (agent scope: global_load / global_store ... sc1) ------------------------------------------------
__device__ __forceinline__ unsigned ld_agent(const void* p) {
    return __hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(void* p, unsigned v) {
    __hip_atomic_store(reinterpret_cast<unsigned*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned long long ld64_agent(const void* p) {
    return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st64_agent(void* p, unsigned long long v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- hand-off: data-tagged granules (MI355X_MICROARCH.md, price list row handoff-1to1) ------------------------------------
__device__ __forceinline__ unsigned hop_tag(unsigned launch) { return launch % 127u + 1u; }

// All waves of the workgroup call this (one barrier inside).  `blk` = the [R][HP] spike block of one frame, written by other
// workgroups of this launch.  Wave k < KS polls the k-th 64-column slice of row tile `rt16` until every word carries `tagw`
// (= tag * 0x02020202; columns >= H are padding, never written, read as zero), parks the masked fragment in LDS (`hb`,
// KS KB); after the barrier every wave reads all KS fragments.  Returns false when the bounded spin expired (error word
// set) -- the wave then stops polling for good (garbage out, the host raises) but keeps executing its barriers.
__device__ __forceinline__ bool hop_gather(const int8_t* blk, int rt16, int R, int KS, int H, unsigned tagw, char* hb, v4i (&b)[HOP_KS_MAX],
                                           bool ok, unsigned* err, int wave, int lane) {
    const int n = lane & 15, q = lane >> 4;
    if (wave < KS) {
        const int row = 16 * rt16 + n, rowc = row < R ? row : R - 1;
        v4i v = {0, 0, 0, 0};
        if (wave * 64 + q * 16 < H) {
            const unsigned* u = reinterpret_cast<const unsigned*>(blk + ((size_t)rowc * KS + wave) * 64 + q * 16);
            for (unsigned spins = 0;; ++spins) {
                bool bad = false;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned w = ld_agent(u + i);
                    bad |= (w & 0xfefefefeu) != tagw;
                    v[i] = (int)(w & 0x01010101u);
                }
                if (!ok || __ballot(bad) == 0) break;
                if (spins > HOP_SPIN_LIMIT) {
                    st_agent(err, 1u);
                    ok = false;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        *reinterpret_cast<v4i*>(hb + (wave * 64 + lane) * 16) = v;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < HOP_KS_MAX; ++ks) {
        b[ks] = v4i{0, 0, 0, 0};
        if (ks < KS) b[ks] = *reinterpret_cast<const v4i*>(hb + (ks * 64 + lane) * 16);
    }
    return ok;
}

#endif
