// The two small algorithms of the replay that must reproduce the reference bit for bit, in one shared form: the frame walk of
// FiguresMix::getTotalPdf (FrameWalk, frame_sum) and the left-first closest walk of BVH::intersect_ (ref_left_first), with the two node readers
// (two_box_node, ref_node).  Nothing here takes a scene: the callers hand in node tables, stacks and leaf bodies, and the test hooks run
// frame_sum on a tree of their own (tests/test_gpu_frame_sum.py) against the model of tests/test_frame_sum_model.py.
#pragma once
#include "rt_device.h"

namespace rtamd {
namespace dev {

// ---- the frame walk ------------------------------------------------------------------------------------------------------------------
// FiguresMix::getTotalPdf (distributions.h:148-165) returns total(left) + total(right) recursively and a sequential sum inside a leaf;
// float addition is not associative, so the same tree of additions is replayed with an explicit frame stack: a TODO(child) frame is the
// right side of a node whose left side is being summed, an ADD(partial) frame the left side's total while the right side is (one tag
// bit per stack slot).  A side that contributes nothing (a failed box, a miss) is +0, the additive identity here: no term is -0.
// What a node says of itself (the `kind` of FrameWalk::down):
enum { FRAME_TOTAL = 0,   // this side's total is v: a leaf's sequential sum, a failed box, or 0
       FRAME_ONE = 1,     // only the side `l` can contribute: go on there, no frame (0 + x is exact)
       FRAME_BOTH = 2 };  // total(l) + total(r): r waits on the stack

// A strided view of a stack kept in memory shared between lanes (entry e of a lane at word e * STRIDE): indexable like an array.
template <int STRIDE> struct StridedStack {
    uint32_t *p;
    RT_DEV uint32_t &operator[](int i) const { return p[STRIDE * i]; }
};

// The walk's state and its two moves.  `stack`: anything indexable that yields a word and holds MAXDEPTH of them.  A FRAME_BOTH at full
// depth counts as a total of 0: the hosts refuse trees deeper than their stacks, so no frame depends on it.
template <int MAXDEPTH> struct FrameWalk {
    static constexpr int WORDS = (MAXDEPTH + 63) / 64;
    int sp = 0;
    unsigned long long add[WORDS] = {};   // frame kind per stack slot: 1 = ADD(partial sum), 0 = TODO(child)
    float v = 0.f;                        // the total of the side just finished
    uint32_t cur = 0;                     // the node to look at next (descending)
    bool descending = true;
    // The words are picked by compares, not by an index: a mask indexed at run time would leave its registers for scratch.
    RT_DEV bool is_add(int i) const {
        bool a = false;
#pragma unroll
        for (int w = 0; w < WORDS; w++)
            if (WORDS == 1 || (i >> 6) == w) a = ((add[w] >> (WORDS == 1 ? i : i & 63)) & 1ull) != 0;
        return a;
    }
    RT_DEV void tag(int i, bool is_add_frame) {
#pragma unroll
        for (int w = 0; w < WORDS; w++)
            if (WORDS == 1 || (i >> 6) == w) {
                const unsigned long long bit = 1ull << (WORDS == 1 ? i : i & 63);
                add[w] = is_add_frame ? add[w] | bit : add[w] & ~bit;
            }
    }
    template <class A> RT_DEV void down(A &&stack, int kind, uint32_t l, uint32_t r) { // for FRAME_TOTAL the caller has set v
        if (kind == FRAME_BOTH && sp >= MAXDEPTH) { v = 0.f; kind = FRAME_TOTAL; }
        if (kind == FRAME_TOTAL) descending = false;
        else {
            if (kind == FRAME_BOTH) { tag(sp, false); stack[sp++] = r; }
            cur = l;
        }
    }
    template <class A> RT_DEV bool up(A &&stack) { // false: the stack is empty, v is the sum
        if (sp == 0) return false;
        --sp;
        const uint32_t f = stack[sp];
        if (is_add(sp)) v = __uint_as_float(f) + v;                                   // left total + right total
        else { tag(sp, true); stack[sp++] = __float_as_uint(v); cur = f; descending = true; }
        return true;
    }
};

// The plain loop over the two moves.  node(cur, l, r, v) -> kind says what the node `cur` is (and sets v, l or l and r accordingly).
template <int MAXDEPTH, class A, class NODE>
RT_DEV float frame_sum(A &&stack, NODE &&node, uint32_t root = 0) {
    FrameWalk<MAXDEPTH> m;
    m.cur = root;
    for (;;) {
        if (m.descending) {
            uint32_t l = 0, r = 0;
            const int kind = node(m.cur, l, r, m.v);
            m.down(stack, kind, l, r);
        } else if (!m.up(stack)) return m.v;
    }
}

// ---- the two node readers --------------------------------------------------------------------------------------------------------
// The library's own two-box nodes (padded boxes, conservative slab test): the left child first, as the reference's light tree has it.
// leaf(first) -> the sequential sum of the leaf's lights from `first` up to the one marked last.
template <class LEAF>
RT_DEV int two_box_node(const GpuNode *nodes, const RayInv &ray, uint32_t cur, uint32_t &l, uint32_t &r, float &v, LEAF &&leaf) {
    if (cur & RT_LEAF_BIT) { v = cur != RT_EMPTY_LEAF ? leaf(cur & ~RT_LEAF_BIT) : 0.f; return FRAME_TOTAL; }
    const float4 *q = reinterpret_cast<const float4 *>(nodes + cur);
    float4 lo0 = q[0], hi0 = q[1], lo1 = q[2], hi1 = q[3];
    float n0, n1;
    bool h0 = slab_test(lo0, hi0, ray, RT_T_MAX, n0);
    bool h1 = slab_test(lo1, hi1, ray, RT_T_MAX, n1);
    l = __float_as_uint(lo0.w); r = __float_as_uint(lo1.w);
    if (h0 & h1) return FRAME_BOTH;
    if (h0) return FRAME_ONE;
    if (h1) { l = r; return FRAME_ONE; }
    v = 0.f;
    return FRAME_TOTAL;
}

// AABB::intersect -> intersectBoxAndRay(0.5 * (max - min), ray - 0.5 * (min + max), false), primitives.cpp:163-165,29-53.
RT_DEV bool ref_box_test(F3 mn, F3 mx, F3 o, F3 d, float &t, bool &inside) {
    const F3 s = 0.5f * (mx - mn);
    const F3 oc = o - 0.5f * (mn + mx);
    const F3 a = neg(s) - oc, b = s - oc;
    const float a1x = a.x / d.x, a1y = a.y / d.y, a1z = a.z / d.z;
    const float a2x = b.x / d.x, a2y = b.y / d.y, a2z = b.z / d.z;
    const float t1x = smin(a1x, a2x), t2x = smax(a1x, a2x);
    const float t1y = smin(a1y, a2y), t2y = smax(a1y, a2y);
    const float t1z = smin(a1z, a2z), t2z = smax(a1z, a2z);
    const float t1 = smax(smax(t1x, t1y), t1z);
    const float t2 = smin(smin(t2x, t2y), t2z);
    if (t1 > t2 || t2 < 0) return false;
    if (t1 < 0) { inside = true; t = t2; }
    else { inside = false; t = t1; }
    return true;
}

struct RefNodeView { F3 mn, mx; uint32_t left, right, first, last; };
RT_DEV RefNodeView load_ref_node(const GpuRefNode *p) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
    const float4 a = q[0], b = q[1], c = q[2];
    RefNodeView n;
    n.mn = f3(a.x, a.y, a.z); n.left = __float_as_uint(a.w);
    n.mx = f3(b.x, b.y, b.z); n.right = __float_as_uint(b.w);
    n.first = __float_as_uint(c.x); n.last = __float_as_uint(c.y);
    return n;
}

// The reference's own nodes with the reference's box test at every one of them (distributions.h:256-262): a failed box contributes 0
// whatever lies below it.  leaf(first, last) -> the sequential sum of the lights first .. last - 1.
template <class LEAF>
RT_DEV int ref_node(const GpuRefNode *nodes, F3 x, F3 d, uint32_t cur, uint32_t &l, uint32_t &r, float &v, LEAF &&leaf) {
    const RefNodeView n = load_ref_node(nodes + cur);
    float tb; bool inside;
    if (!ref_box_test(n.mn, n.mx, x, d, tb, inside)) { v = 0.f; return FRAME_TOTAL; }
    if (n.left == 0) { v = leaf(n.first, n.last); return FRAME_TOTAL; }
    l = n.left; r = n.right;
    return FRAME_BOTH;
}

// ---- the left-first closest walk -----------------------------------------------------------------------------------------------------
// BVH::intersect_ (bvh.h:111-142) as an iterative depth-first walk over the reference's own tree, left child first.  The recursion's
// `curBest` at a node is the smallest t of everything found before the node in this order (every level hands its left result on to its
// right child), so one running best prunes (`curBest < t_box && !inside`, bvh.h:118); a leaf keeps its first figure on equal t and a later
// subtree replaces the best only when strictly closer, so the leaf bodies lower `best` on strict '<' only.
// leaf(first, last) tests the figures first .. last - 1 and lowers `best`; `stack` holds MAXDEPTH node indices (deeper: see FrameWalk).
struct RefBest { bool have; float t; };
template <int MAXDEPTH, class A, class LEAF>
RT_DEV void ref_left_first(const GpuRefNode *nodes, F3 o, F3 d, A &&stack, RefBest &best, LEAF &&leaf) {
    int sp = 0;
    uint32_t cur = 0;
    for (;;) {
        const RefNodeView n = load_ref_node(nodes + cur);
        float tb; bool inside;
        if (ref_box_test(n.mn, n.mx, o, d, tb, inside) && !(best.have && best.t < tb && !inside)) {
            if (n.left == 0) leaf(n.first, n.last);
            else if (sp < MAXDEPTH) { stack[sp++] = n.right; cur = n.left; continue; }
        }
        if (sp == 0) break;
        cur = stack[--sp];
    }
}

} // namespace dev
} // namespace rtamd
