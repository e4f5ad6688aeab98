// The round pipeline's path state as the kernels see it (rt_wavefront.h: record layout, queues); the scene object keeps one across renders.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtamd {
namespace dev {

struct WfView {
    float4 *r0;             // per slot: `stride` float4 = WF_REC_BASE (R0 record) + 2 per stack level, contiguous
    uint32_t stride;
    uint32_t *q_trace[2];
    uint32_t *q_light;
    uint32_t *ctr;          // per round r, WF_CTR words: +0 trace count, +1 light count, +2 trace head, +3 light head, +4 slow-light count
    uint32_t *q_slow;       // light queries of this round that the lean walker hands to wf_light_exact_kernel
    uint32_t n_slots;
    uint32_t *ovf;          // SPILL variant only: WF_OVF stack entries per persistent thread beyond the WF_STACK entries in LDS
    uint32_t slot_base;     // this pipeline's first path slot (the frame's slots are cut into independent pipelines, one per stream)
};

} // namespace dev
} // namespace rtamd
