// ORACLE — TEST INFRASTRUCTURE ONLY (see oracle_common.h).
// The SAH tree of the hw5 / hw6 / hw8 snapshots, restated once: boxes, the builder, the left-first closest-hit walk and the
// light-pdf sum (hw5/src/include/bvh.h:18-141, hw6/src/include/bvh.h, hw8/src/include/bvh.h:9-142).  The three snapshots' trees
// differ in four places only, which a Traits class supplies:
//   Traits::Hit                      the snapshot's own intersection record
//   Traits::box_of(const Fig &)      the figure's box
//   Traits::key(const Fig &)         the V3 whose coordinates half_split sorts on (Figure::position in hw5 / hw6, data3.coords in hw8)
//   Traits::hit(fig, o, d, Hit &)    the leaf's figure test
//   Traits::count_box()              called once per box test (the counting oracles hw6 / hw8 tally; hw5 does nothing)
#pragma once
#include "oracle_common.h"
#include <utility>

namespace rto {

struct Box { V3 mn, mx; };

// AABB::extend — hw5/src/primitives.cpp:204-211, hw8/src/primitives.cpp:144-156
static inline void extend(Box &b, V3 p) {
    b.mx.x = smax(b.mx.x, p.x); b.mx.y = smax(b.mx.y, p.y); b.mx.z = smax(b.mx.z, p.z);
    b.mn.x = smin(b.mn.x, p.x); b.mn.y = smin(b.mn.y, p.y); b.mn.z = smin(b.mn.z, p.z);
}
static inline void extend(Box &b, const Box &o) { extend(b, o.mn); extend(b, o.mx); }
// hw8/src/primitives.cpp:158-161
static inline float surf(const Box &b) {
    V3 d = b.mx - b.mn;
    return 2 * (d.x * d.y + d.x * d.z + d.y * d.z);
}
// intersectBoxAndRay with require_norma == false, the only form the trees use
// (hw5/src/primitives.cpp:91-115, hw6/src/primitives.cpp:92-116, hw8/src/primitives.cpp:29-53)
static inline bool slab_ray(V3 s, V3 o, V3 d, float &t, bool &inside) {
    V3 ts1 = (neg1(s) - o) / d;
    V3 ts2 = (s - o) / d;
    float t1x = smin(ts1.x, ts2.x), t2x = smax(ts1.x, ts2.x);
    float t1y = smin(ts1.y, ts2.y), t2y = smax(ts1.y, ts2.y);
    float t1z = smin(ts1.z, ts2.z), t2z = smax(ts1.z, ts2.z);
    float t1 = smax(smax(t1x, t1y), t1z);
    float t2 = smin(smin(t2x, t2y), t2z);
    if (t1 > t2 || t2 < 0) return false;
    if (t1 < 0) { inside = true; t = t2; }
    else { inside = false; t = t1; }
    return true;
}
// AABB::intersect — hw5/src/primitives.cpp:220-222, hw6/src/primitives.cpp:221-223, hw8/src/primitives.cpp:163-165
static inline bool aabb_ray(const Box &b, V3 o, V3 d, float &t, bool &inside) {
    return slab_ray(0.5f * (b.mx - b.mn), o - 0.5f * (b.mn + b.mx), d, t, inside);
}

struct Node { Box aabb; uint32_t left = 0, right = 0, first = 0, last = 0; }; // bvh.h:9-16

template <class Fig, class Traits> struct Bvh {
    typedef typename Traits::Hit Hit;
    std::vector<Node> nodes;
    uint32_t root = 0;
    uint32_t depth = 0;

    // hw8 bvh.h:34-54
    static std::pair<float, uint32_t> best_split(std::vector<Fig> &figs, uint32_t first, uint32_t last) {
        std::vector<float> scores(last - first, 0);
        Box pre = Traits::box_of(figs[first]);
        for (size_t i = 1; i < last - first; i++) {
            scores[i] = surf(pre) * i;
            extend(pre, Traits::box_of(figs[first + i]));
        }
        Box suf = Traits::box_of(figs[last - 1]);
        for (size_t i = last - first - 1; i >= 1; i--) {
            scores[i] += surf(suf) * ((last - first) - i);
            extend(suf, Traits::box_of(figs[first + i - 1]));
        }
        std::pair<float, uint32_t> ans = {scores[1], first + 1};
        for (size_t i = 2; i < last - first; i++)
            if (scores[i] < ans.first) ans = {scores[i], (uint32_t)(first + i)};
        return ans;
    }
    // hw8 bvh.h:60-65, hw5 / hw6 bvh.h:61-63.  std::sort, not stable_sort: where keys tie (every key, in hw6) the order left behind
    // is whatever introsort's sequence of comparisons gives.
    static void half_split(std::vector<Fig> &figs, uint32_t first, uint32_t last, int axis) {
        if (axis == 0) std::sort(figs.begin() + first, figs.begin() + last, [](const Fig &l, const Fig &r) { return Traits::key(l).x < Traits::key(r).x; });
        else if (axis == 1) std::sort(figs.begin() + first, figs.begin() + last, [](const Fig &l, const Fig &r) { return Traits::key(l).y < Traits::key(r).y; });
        else std::sort(figs.begin() + first, figs.begin() + last, [](const Fig &l, const Fig &r) { return Traits::key(l).z < Traits::key(r).z; });
    }
    // hw8 bvh.h:67-109
    uint32_t build(std::vector<Fig> &figs, uint32_t first, uint32_t last, uint32_t d = 1) {
        if (d > depth) depth = d;
        Node cur; cur.first = first; cur.last = last;
        Box aabb;
        if (first < last) aabb = Traits::box_of(figs[first]);
        for (uint32_t i = first + 1; i < last; i++) extend(aabb, Traits::box_of(figs[i]));
        cur.aabb = aabb;
        uint32_t pos = (uint32_t)nodes.size();
        nodes.push_back(cur);
        if (last - first <= 1) return pos;
        half_split(figs, first, last, 0); auto sx = best_split(figs, first, last);
        half_split(figs, first, last, 1); auto sy = best_split(figs, first, last);
        half_split(figs, first, last, 2); auto sz = best_split(figs, first, last);
        float best = smin(sx.first, smin(sy.first, sz.first));
        if (best >= surf(aabb) * (last - first)) return pos;
        uint32_t mid;
        if (best == sx.first) { mid = sx.second; half_split(figs, first, last, 0); }
        else if (best == sy.first) { mid = sy.second; half_split(figs, first, last, 1); }
        else { mid = sz.second; half_split(figs, first, last, 2); }
        uint32_t l = build(figs, first, mid, d + 1); nodes[pos].left = l;
        uint32_t r = build(figs, mid, last, d + 1); nodes[pos].right = r;
        return pos;
    }
    void init(std::vector<Fig> &figs, uint32_t n) { nodes.clear(); depth = 0; root = build(figs, 0, n); }

    // hw8 bvh.h:111-142, hw5 bvh.h:111-140 — recursive closest hit, left child first, strict '<' keeps the first found.
    bool intersect(const std::vector<Fig> &figs, uint32_t pos, V3 o, V3 d, bool have_best, float cur_best, Hit &out, int &idx) const {
        const Node &cur = nodes[pos];
        float t; bool inside;
        Traits::count_box();
        if (!aabb_ray(cur.aabb, o, d, t, inside)) return false;
        if (have_best && cur_best < t && !inside) return false;
        bool found = false;
        if (cur.left == 0) {
            for (uint32_t i = cur.first; i < cur.last; i++) {
                Hit h;
                if (Traits::hit(figs[i], o, d, h) && (!found || h.t < out.t)) { out = h; idx = (int)i; found = true; }
            }
            return found;
        }
        Hit lh; int li = -1;
        bool lf = intersect(figs, cur.left, o, d, have_best, cur_best, lh, li);
        if (lf) { out = lh; idx = li; found = true; }
        if (lf && (!have_best || lh.t < cur_best)) { cur_best = lh.t; have_best = true; }
        Hit rh; int ri = -1;
        bool rf = intersect(figs, cur.right, o, d, have_best, cur_best, rh, ri);
        if (rf && (!found || rh.t < out.t)) { out = rh; idx = ri; found = true; }
        return found;
    }

    // FiguresMix::getTotalPdf over a tree of lights — hw5/src/include/distributions.h:256-274, hw6 :239-256, hw8 :148-165.
    // one_light(i) is the pdf term of light i (pdfOneFigureLight); leaves add theirs in order, then left + right.
    template <class OneLight> float total_pdf(uint32_t pos, V3 x, V3 d, OneLight &&one_light) const {
        const Node &cur = nodes[pos];
        float t; bool inside;
        Traits::count_box();
        if (!aabb_ray(cur.aabb, x, d, t, inside)) return 0;
        if (cur.left == 0) {
            float result = 0;
            for (uint32_t i = cur.first; i < cur.last; i++) result += one_light(i);
            return result;
        }
        float l = total_pdf(cur.left, x, d, one_light);
        float r = total_pdf(cur.right, x, d, one_light);
        return l + r;
    }
};

} // namespace rto
