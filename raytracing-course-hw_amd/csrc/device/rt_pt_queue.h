// The work queues of the persistent kernels (rt_persistent.h, rt_persistent_hw6.h): one bit per path in an LDS bitmap and a counter beside it.
// pt_push sets bits, pt_pop hands the set bits of a sweep to the lanes of a wave that want a path.  Nothing here knows the scene or the
// kernels: the test hooks run pt_pop on a bitmap of their own (tests/test_gpu_pt_pop.py) against the model of tests/test_pt_pop_model.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef RT_DEV
#define RT_DEV __device__ __forceinline__
#endif
#define PT_NONE 0xFFFFFFFFu

namespace rtamd {
namespace dev {

// ---- bit helpers (host and device) -------------------------------------------------------------------------------------------------
// Position of the n-th set bit of v, n counted from 0 (n < popcount(v)): a binary search on the counts of the lower halves, five steps
// whatever v holds.
__host__ __device__ inline int pt_nth_bit(uint32_t v, int n) {
    int pos = 0;
#pragma unroll
    for (int h = 16; h > 0; h >>= 1) {
        const int c = __builtin_popcount((v >> pos) & ((1u << h) - 1u));
        if (n >= c) { n -= c; pos += h; }
    }
    return pos;
}
// The lowest n set bits of v (1 <= n <= popcount(v)).
__host__ __device__ inline uint32_t pt_low_bits(uint32_t v, int n) { return v & ((2u << pt_nth_bit(v, n - 1)) - 1u); }

// ---- wave-level helpers ------------------------------------------------------------------------------------------------------------
// A fresh LDS read each time; every lane reads the same word, and readfirstlane makes that explicit: the scheduler's decisions are
// taken on SGPRs (scalar branches, wave-uniform by construction — the code under them uses __ballot / __shfl / lane-0 atomics).
RT_DEV int pt_count(const int *p) { return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)); }

// The wave's mask of a predicate, straight from the compare (HIP's __ballot takes an int: a select and a second compare per call).
RT_DEV unsigned long long pt_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// Number of set bits of a wave mask below this lane (v_mbcnt: no 64-bit lane mask in registers).
RT_DEV uint32_t pt_rank_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// x of the lane `ctrl` names (a DPP control: 0x110 + n = n lanes down in the row of 16, 0x142 / 0x143 = lane 15 of the row before / lane
// 31), 0 where there is no such lane or the lane's row is not in row_mask.
template <int CTRL, int ROW_MASK> RT_DEV int pt_dpp_or_zero(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xf, false); }
// Exclusive prefix sum over the wave of a count per lane, without LDS: a scan on the DPP lanes — four steps inside the rows of 16, then
// lane 15 of rows 0 and 2 to the rows after them and lane 31 to the upper half.  Six adds whatever the counts are.  All 64 lanes must
// be active (a DPP read of an inactive lane gives 0).  `total` is wave-uniform.
RT_DEV int pt_prefix(int x, int &total) {
    int s = x;
    s += pt_dpp_or_zero<0x111, 0xf>(s);
    s += pt_dpp_or_zero<0x112, 0xf>(s);
    s += pt_dpp_or_zero<0x114, 0xf>(s);
    s += pt_dpp_or_zero<0x118, 0xf>(s);
    s += pt_dpp_or_zero<0x142, 0xa>(s);
    s += pt_dpp_or_zero<0x143, 0xc>(s);
    total = __builtin_amdgcn_readlane(s, 63);
    return s - x;
}

// Counting builds: what the pops of one queue handed out.  paths / pops tells a dense queue from a sparse one, words / pops what the deal costs.
struct PtPopStat {
    unsigned long long pops = 0, paths = 0, words = 0; // calls | paths handed out | bitmap words they came from
};

// Hands paths to the lanes that want one.  The wave reads 64 bitmap words at once (lane i: word cursor + i), then the words
// claim for themselves — one LDS atomic instruction for all of them — and the claimed bits are dealt to the wanting lanes by rank, so a wave that
// wants 64 paths from a dense queue gets the two words of one 8x8 sub-tile (coherent rays) for two LDS atomics.  A word that
// holds more paths than are wanted keeps its upper bits and the cursor stays on it, so the next request starts there (no
// path is passed over).  Returns the local path index or PT_NONE.
// from_start: every request sweeps from word 0 — the paths at the front of the workgroup's list (its most expensive sub-tiles after a
// re-deal) are always served first, so the longest serial chains (a pixel's samples are serial) never wait behind cheap work.
//
// The deal takes the same time whatever the words hold.  A claimed word is wave-uniform once it is read from its lane, so lane i < 32
// stands for its bit i: the lane's rank among the set bits (v_mbcnt) is the rank of the wanting lane the path goes to, and one ds_permute
// per word sends path + 1 to the lane of that number (`box`); the lanes that stand for no path send 0 to the lane behind the word's last
// rank, which no path of this word goes to.  Words take disjoint ranks, so the boxes are merged with an OR, and after the sweep every
// wanting lane fetches the box of its rank with one ds_bpermute.  The only search for an n-th bit left is the one word that is cut
// (pt_low_bits).  The OR rests on two things: at most 64 lanes want, so every rank is a lane number below 64, and ds_permute returns 0 in a
// lane that nobody wrote to.  Every caller enters with all 64 lanes active and wave-uniform arguments (but `want`), and every cross-lane operation
// here (ballots, DPP scan, readlane, permutes) stands outside divergent code: it needs the whole wave.
RT_DEV uint32_t pt_pop(uint32_t *bm, int *cnt, const uint32_t nw, uint32_t &cursor, bool want, bool from_start = false, PtPopStat *stat = nullptr) {
    const uint32_t lane = threadIdx.x & 63u;
    if (from_start) cursor = 0u;
    const unsigned long long wantmask = pt_ballot(want);
    const int need = __popcll(wantmask);
    uint32_t box = 0u;                                                // lane r: 1 + the path of the wanting lane of rank r, 0 = none
    int have = 0;                                                 // wave-uniform, like everything below that is not per word (= per lane) or `box`
    for (uint32_t swept = 0; swept < nw && have < need; swept += 64u) {
        uint32_t w = cursor + lane;
        const bool valid = lane < nw;                                 // fewer than 64 words: the wave sees the whole ring at once
        if (w >= nw) w -= nw;                                         // cursor < nw, and lane < nw where the word is read: no division
        const uint32_t v = valid ? bm[w] : 0u;
        // Every word claims for itself, all in ONE LDS atomic of the wave: word i may take what the words before it leave of the request
        // (a prefix sum of the words' bit counts).  A claim can come back short (another wave was faster); the sweep then goes on.
        const int pc = __popc(v);
        int in_sight;
        const int before = pt_prefix(pc, in_sight);
        uint32_t next_cursor = cursor + 64u;
        if (in_sight) {
            const int open = need - have, room = open - before;
            uint32_t take = 0u;
            if (pc > 0 && room > 0) take = room < pc ? pt_low_bits(v, room) : v; // the one word that is cut: its lowest `room` set bits
            uint32_t old = 0u;
            if (take) old = atomicAnd(&bm[w], ~take) & take;     // the bits this word really gave
            // This word's paths go to the wanting lanes of ranks have + first, ...  Where every claim came back whole the words gave what
            // they were asked for, and the prefix sum of that is known; a short claim takes a scan of what they did give.
            int claimed = in_sight < open ? in_sight : open, first = before < open ? before : open;
            if (pt_ballot(old != take)) first = pt_prefix(__popc(old), claimed);
            const unsigned long long cm = pt_ballot(old != 0u);
            for (unsigned long long m = cm; m; m &= m - 1ull) {
                const int j = __ffsll((long long)m) - 1;
                const uint32_t oj = (uint32_t)__builtin_amdgcn_readlane((int)old, j), wj = (uint32_t)__builtin_amdgcn_readlane((int)w, j);
                const uint32_t fj = (uint32_t)(have + __builtin_amdgcn_readlane(first, j));
                const bool mine = __builtin_amdgcn_inverse_ballot_w64((unsigned long long)oj); // the word as a lane mask: lane i < 32 holds bit i
                const uint32_t rank = __builtin_amdgcn_mbcnt_lo(oj, fj), behind = (fj + (uint32_t)__popc(oj)) & 63u; // both computed: one select, no branch
                const uint32_t to = mine ? rank : behind;
                box |= (uint32_t)__builtin_amdgcn_ds_permute((int)(to << 2), mine ? (int)(wj * 32u + lane + 1u) : 0);
            }
            have += claimed;
            if (stat) stat->words += __popcll(cm);
            const unsigned long long tm = pt_ballot(take != 0u);
            if (tm && have >= need) {                             // done: the next request starts at the last word touched if it kept paths, else behind it
                const int jl = 63 - __clzll((long long)tm);
                const uint32_t wl = (uint32_t)__builtin_amdgcn_readlane((int)w, jl), left = (uint32_t)__builtin_amdgcn_readlane((int)(v & ~take), jl);
                next_cursor = left ? wl : wl + 1u;
            }
        }
        cursor = (uint32_t)__builtin_amdgcn_readfirstlane((int)next_cursor);
        while (cursor >= nw) cursor -= nw;                            // cursor % nw on SGPRs; one round, but for a ring of under 64 words swept without finding enough
    }
    if (have && lane == 0) atomicSub(cnt, have);
    if (stat) { stat->pops++; stat->paths += (unsigned long long)have; }
    const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(pt_rank_below(wantmask) << 2), (int)box) - 1u; // box 0 -> PT_NONE
    return want ? got : PT_NONE;
}

// Sets the bit of path l in queue q for the lanes with `doit` (wave-uniform call).
template <class SH> RT_DEV void pt_push(SH &sh, int q, uint32_t l, bool doit) {
    if (doit) atomicOr(&sh.need[q][l >> 5], 1u << (l & 31u));
    const unsigned long long m = pt_ballot(doit);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(&sh.cnt[q], (int)__popcll(m));
}

} // namespace dev
} // namespace rtamd
