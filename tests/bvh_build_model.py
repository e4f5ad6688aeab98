"""The on-device scene-tree builder (csrc/device/rt_bvh_build.h, driver csrc/rtamd_build.hip) restated in numpy: float32 with one rounding
per operation, exactly the kernels' operations in their order, so that every node word, the leaf order, the leaf marks and the depth can be
compared bit for bit.  The builder is deterministic by construction (integer atomicMax / atomicAdd, a sequential sweep per node, prefix-sum
numbering, leaves sorted by load index, no contraction), so a level is restated for all its open nodes at once: every array below has the
level's open nodes (in bin-slot order) as its first axis, and the sweeps loop over axis, then plane, as the one thread per node does.

check_tree is the other half: the invariants of a valid tree, checked on the emitted arrays alone, without the model."""
import numpy as np

F, U = np.float32, np.uint32
BINS, MAX_LEAF, MAX_DEPTH, LDS_NODES, THREADS = 16, 8, 28, 32, 1024   # BVB_BINS, BVB_MAX_LEAF, BVB_MAX_DEPTH, BVB_LDS_NODES, BVB_THREADS
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF
BIG = F(3.0e38)                                                        # the sweeps' start value and the empty child's box
TALLY = ("leaf_by_sah", "hash_split", "closed_by_depth", "guard_overrode", "unsplit_hash_half_empty")


def ord_key(f):
    """bvb_ord: floats to integers of the same order; -0.0 sorts below +0.0, as the atomicMax sees them."""
    b = np.ascontiguousarray(f, F).view(U)
    return np.where(b & U(0x80000000), ~b, b | U(0x80000000)).astype(U)


def unord(u):
    u = np.ascontiguousarray(u, U)
    return np.where(u & U(0x80000000), u & U(0x7FFFFFFF), ~u).astype(U).view(F)


def hash_bit(p, depth):
    """bvb_hash_bit: the bit of the index hash that halves a node at `depth` when no plane separates its centroids."""
    m = np.uint64(0xFFFFFFFF)
    h = (np.asarray(p).astype(np.uint64) * np.uint64(0x9E3779B1)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    return ((h >> (np.asarray(depth).astype(np.uint64) & np.uint64(31))) & np.uint64(1)).astype(np.int64)


def to_int(x):
    """(int)x as v_cvt_i32_f32 converts: toward zero, saturating, NaN gives 0 (C++ leaves NaN and out-of-range values undefined)."""
    x = np.asarray(x, F)
    t = np.trunc(np.clip(np.where(np.isnan(x), F(0), x), F(-2147483648.0), F(2147483520.0)).astype(np.float64))
    return np.where(x >= F(2147483648.0), 2147483647, t).astype(np.int64)


def bin_of(c2, clo2, chi2):
    """bvb_bin: twice the centroid against the node's doubled centroid bounds.  A denormal extent makes 16 / e infinite: the centroid on
    the lower bound then gives 0 * inf = NaN and bin 0, every other one +inf and bin 15."""
    with np.errstate(all="ignore"):
        e = (chi2 - clo2).astype(F)
        b = to_int(((c2 - clo2).astype(F) * (F(BINS) / e).astype(F)).astype(F))
        return np.where(e > F(0), np.clip(b, 0, BINS - 1), 0)


def half_area(lo, hi):
    with np.errstate(all="ignore"):
        ex, ey, ez = hi[..., 0] - lo[..., 0], hi[..., 1] - lo[..., 1], hi[..., 2] - lo[..., 2]
        return ((ex * ey + ey * ez) + ez * ex).astype(F)


def pad_box(lo, hi, abs_pad):
    """bvb_pad_box: mag * 2^-17 + abs_pad + 1e-30f, added left to right."""
    with np.errstate(all="ignore"):
        mag = np.fmax(np.abs(lo), np.abs(hi)).astype(F)
        pad = ((mag * F(7.62939453125e-06) + F(abs_pad)) + F(1e-30)).astype(F)
        return (lo - pad).astype(F), (hi + pad).astype(F)


def split_boxes(boxes):
    b = np.ascontiguousarray(boxes, F).reshape(-1, 8)
    return b[:, 0:3].copy(), b[:, 4:7].copy()


def build(boxes, abs_pad, max_depth):
    """Returns a dict: nodes (n_nodes, 16) uint32, order, last, depth, n_nodes; open_per_level (open nodes of every level that had any),
    tally (TALLY's branches), n_builder_nodes, and hash_events: (depth, primitives, was split) of every node that came to the hash split."""
    lo, hi = split_boxes(boxes)
    n = len(lo)
    assert n >= 1 and 8 <= max_depth <= MAX_DEPTH
    with np.errstate(all="ignore"):
        c2 = (lo + hi).astype(F)
    klo, khi, kc = ord_key(lo), ord_key(hi), ord_key(c2)
    cap = 2 * n + 2
    n_lo, n_hi = np.zeros((cap, 3), F), np.zeros((cap, 3), F)
    n_count, n_left, n_depth = np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.int64)
    n_cmin, n_cmax = np.full((cap, 3), 0xFFFFFFFF, U), np.zeros((cap, 3), U)       # centroid bounds as keys (min of ord, max of ord)
    n_lo[0], n_hi[0] = unord(klo.min(axis=0)), unord(khi.max(axis=0))               # bvb_init_kernel, bvb_root_kernel
    n_cmin[0], n_cmax[0] = kc.min(axis=0), kc.max(axis=0)
    n_count[0] = n
    n_nodes = 1
    prim_node = np.zeros(n, np.int64)
    open_cur = np.array([0], np.int64) if n > 1 else np.zeros(0, np.int64)
    open_per_level, hash_events = [], []
    tally = dict.fromkeys(TALLY, 0)
    ax3 = np.arange(3)[None, :]

    for level in range(max_depth + 1):
        R = len(open_cur)
        if R == 0:
            break
        open_per_level.append(R)
        rank_of = np.full(n_nodes, -1, np.int64)
        rank_of[open_cur] = np.arange(R)
        pr = rank_of[prim_node]
        sel = np.flatnonzero(pr >= 0)
        r = pr[sel]
        depth, count = n_depth[open_cur], n_count[open_cur]
        # ---- bvb_bin_kernel
        bins = bin_of(c2[sel], unord(n_cmin[open_cur])[r], unord(n_cmax[open_cur])[r])               # (m, 3)
        cnt = np.zeros((R, 3, BINS), np.int64)
        np.add.at(cnt, (r[:, None], ax3, bins), 1)
        kmin, kmax = np.full((R, 3, BINS, 3), 0xFFFFFFFF, U), np.zeros((R, 3, BINS, 3), U)
        np.minimum.at(kmin, (r[:, None], ax3, bins), klo[sel][:, None, :])
        np.maximum.at(kmax, (r[:, None], ax3, bins), khi[sel][:, None, :])
        blo, bhi = unord(kmin), unord(kmax)                                                          # garbage where a bin is empty: never read
        hb = hash_bit(sel, depth[r])
        hcnt = np.zeros((R, 2), np.int64)
        np.add.at(hcnt, (r, hb), 1)
        # ---- bvb_split_kernel
        best, bal_best = np.full(R, BIG, F), np.full(R, BIG, F)
        best_axis, best_plane = np.full(R, -1, np.int64), np.zeros(R, np.int64)
        bal_axis, bal_plane = np.full(R, -1, np.int64), np.zeros(R, np.int64)
        with np.errstate(all="ignore"):
            for k in range(3):
                w_cnt, w_lo, w_hi = cnt[:, k], blo[:, k], bhi[:, k]
                s_lo, s_hi, c = np.full((R, 3), BIG, F), np.full((R, 3), -BIG, F), np.zeros(R, np.int64)
                r_cnt, r_area = np.zeros((R, BINS), np.int64), np.zeros((R, BINS), F)
                for i in range(BINS - 1, 0, -1):                                                     # suffix: bins i .. 15
                    m = (w_cnt[:, i] > 0)[:, None]
                    s_lo, s_hi = np.where(m, np.fmin(s_lo, w_lo[:, i]), s_lo), np.where(m, np.fmax(s_hi, w_hi[:, i]), s_hi)
                    c = c + w_cnt[:, i]
                    r_cnt[:, i], r_area[:, i] = c, np.where(c > 0, half_area(s_lo, s_hi), F(0))
                s_lo, s_hi, c = np.full((R, 3), BIG, F), np.full((R, 3), -BIG, F), np.zeros(R, np.int64)
                for i in range(BINS - 1):                                                            # plane i: bins 0..i | i+1..15
                    m = (w_cnt[:, i] > 0)[:, None]
                    s_lo, s_hi = np.where(m, np.fmin(s_lo, w_lo[:, i]), s_lo), np.where(m, np.fmax(s_hi, w_hi[:, i]), s_hi)
                    c = c + w_cnt[:, i]
                    cr = r_cnt[:, i + 1]
                    valid = (c > 0) & (cr > 0)
                    cost = ((half_area(s_lo, s_hi) * c.astype(F)).astype(F) + (r_area[:, i + 1] * cr.astype(F)).astype(F)).astype(F)
                    upd = valid & (cost < best)                                                      # strict, first wins; a NaN cost never
                    best, best_axis, best_plane = np.where(upd, cost, best), np.where(upd, k, best_axis), np.where(upd, i, best_plane)
                    bal = np.abs(c.astype(F) - cr.astype(F)).astype(F)
                    upd = valid & (bal < bal_best)
                    bal_best, bal_axis, bal_plane = np.where(upd, bal, bal_best), np.where(upd, k, bal_axis), np.where(upd, i, bal_plane)
            found = best_axis >= 0
            halves = (hcnt[:, 0] > 0) & (hcnt[:, 1] > 0)
            want_hash = ~found & (count > MAX_LEAF) & (depth < max_depth)
            by_hash = want_hash & halves
            sah_leaf = found & (count <= MAX_LEAF) & ~(best < (half_area(n_lo[open_cur], n_hi[open_cur]) * count.astype(F)).astype(F))
            split = found & ~sah_leaf
            at_limit = depth >= max_depth
            tally["leaf_by_sah"] += int(sah_leaf.sum())
            tally["closed_by_depth"] += int((at_limit & (split | (~found & (count > MAX_LEAF) & halves))).sum())
            tally["hash_split"] += int(by_hash.sum())
            tally["unsplit_hash_half_empty"] += int((want_hash & ~halves).sum())
            split &= ~at_limit
            shift = np.clip(max_depth - depth - 2, 0, 62)
            guard = split & (depth + 2 < max_depth) & (count * 4 > (np.int64(1) << shift) * MAX_LEAF)
            tally["guard_overrode"] += int((guard & ((bal_axis != best_axis) | (bal_plane != best_plane))).sum())
            axis, plane = np.where(guard, bal_axis, best_axis), np.where(guard, bal_plane, best_plane)
        for q in np.flatnonzero(want_hash):
            hash_events.append((int(depth[q]), np.sort(sel[r == q]), bool(by_hash[q])))
        # the children's boxes along the chosen axis
        rows, a = np.arange(R), np.clip(axis, 0, 2)
        w_cnt, w_lo, w_hi = cnt[rows, a], blo[rows, a], bhi[rows, a]
        llo, lhi, rlo, rhi = np.full((R, 3), BIG, F), np.full((R, 3), -BIG, F), np.full((R, 3), BIG, F), np.full((R, 3), -BIG, F)
        nl, nr = np.zeros(R, np.int64), np.zeros(R, np.int64)
        for i in range(BINS):
            some = w_cnt[:, i] > 0
            ml, mr = (some & (i <= plane))[:, None], (some & (i > plane))[:, None]
            llo, lhi = np.where(ml, np.fmin(llo, w_lo[:, i]), llo), np.where(ml, np.fmax(lhi, w_hi[:, i]), lhi)
            rlo, rhi = np.where(mr, np.fmin(rlo, w_lo[:, i]), rlo), np.where(mr, np.fmax(rhi, w_hi[:, i]), rhi)
            nl, nr = nl + np.where(ml[:, 0], w_cnt[:, i], 0), nr + np.where(mr[:, 0], w_cnt[:, i], 0)
        h = by_hash[:, None]                                                                         # both halves keep the node's box
        llo, lhi = np.where(h, n_lo[open_cur], llo), np.where(h, n_hi[open_cur], lhi)
        rlo, rhi = np.where(h, n_lo[open_cur], rlo), np.where(h, n_hi[open_cur], rhi)
        nl, nr = np.where(by_hash, hcnt[:, 0], nl), np.where(by_hash, hcnt[:, 1], nr)
        axis, plane = np.where(by_hash, 3, axis), np.where(by_hash, 0, plane)
        split |= by_hash
        # ---- bvb_number_kernel: children in the order of their parents, bin slots in the order left, right
        s = np.flatnonzero(split)
        left = n_nodes + 2 * np.arange(len(s))
        n_left[open_cur[s]] = left
        for side, (clo_, chi_, cn) in enumerate(((llo, lhi, nl), (rlo, rhi, nr))):
            n_lo[left + side], n_hi[left + side], n_count[left + side], n_depth[left + side] = clo_[s], chi_[s], cn[s], depth[s] + 1
        children = np.stack([left, left + 1], axis=1).reshape(-1)
        n_nodes += 2 * len(s)
        open_next = children[n_count[children] > 1]
        # ---- bvb_assign_kernel
        moved = split[r]
        p, q = sel[moved], r[moved]
        go_right = np.where(axis[q] == 3, hb[moved], (bins[moved][np.arange(len(p)), np.clip(axis[q], 0, 2)] > plane[q]).astype(np.int64))
        child = n_left[open_cur[q]] + go_right
        prim_node[p] = child
        np.minimum.at(n_cmin, child, kc[p])
        np.maximum.at(n_cmax, child, kc[p])
        open_cur = open_next
    assert len(open_cur) == 0

    # ---- bvb_layout_kernel, bvb_place_kernel, bvb_emit_kernel, bvb_marks_kernel
    is_leaf = n_left[:n_nodes] == 0
    leaf_cnt = np.where(is_leaf, n_count[:n_nodes], 0)
    first = np.cumsum(leaf_cnt) - leaf_cnt                                 # a leaf's first slot: leaves in node order
    inner = np.cumsum(~is_leaf) - (~is_leaf)                               # an inner node's index: inner nodes in node order
    n_inner = int((~is_leaf).sum())
    assert int(leaf_cnt.sum()) == n
    order = np.lexsort((np.arange(n), first[prim_node])).astype(U)         # leaves sorted by load index
    last = np.zeros(n, np.uint8)
    last[(first + leaf_cnt - 1)[is_leaf & (leaf_cnt > 0)]] = 1
    words = np.zeros((max(n_inner, 1), 16), U)
    if n_nodes == 1:                                                       # the root is a leaf: wrapped, the other child empty
        plo, phi = pad_box(n_lo[0], n_hi[0], abs_pad)
        words[0, 0:3], words[0, 3], words[0, 4:7], words[0, 7] = plo.view(U), LEAF | 0, phi.view(U), n
        words[0, 8:11], words[0, 11], words[0, 12:15], words[0, 15] = BIG.view(U), EMPTY, BIG.view(U), 0
    else:
        i = np.flatnonzero(~is_leaf)
        for side in (0, 1):
            ch = n_left[i] + side
            plo, phi = pad_box(n_lo[ch], n_hi[ch], abs_pad)
            o = 8 * side
            words[inner[i], o:o + 3], words[inner[i], o + 4:o + 7] = plo.view(U), phi.view(U)
            words[inner[i], o + 3] = np.where(is_leaf[ch], LEAF | first[ch], inner[ch]).astype(U)
            words[inner[i], o + 7] = np.where(is_leaf[ch], n_count[ch], 0).astype(U)
    return dict(nodes=words, order=order, last=last, depth=int(n_depth[:n_nodes][is_leaf].max()), n_nodes=max(n_inner, 1),
                open_per_level=open_per_level, tally=tally, n_builder_nodes=n_nodes, hash_events=hash_events)


# ---- the structural check: nothing of the above but the formats ------------------------------------------------------------------------
def _padded(lo, hi, abs_pad):
    """The emitted box of a float32 box: each side moved out by max(|lo|, |hi|) * 2^-17 + abs_pad + 1e-30 (scene_prep.cpp pad_box), in float32."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    with np.errstate(all="ignore"):
        pad = np.maximum(np.abs(lo), np.abs(hi)) * np.float32(2.0 ** -17)
        pad = pad + np.float32(abs_pad)
        pad = pad + np.float32(1e-30)
        return lo - pad, hi + pad


def check_tree(boxes, abs_pad, max_depth, nodes, order, last, depth):
    """Asserts that (nodes, order, last, depth) is a valid tree of the builder's kind over `boxes`; every message names the node."""
    blo, bhi = split_boxes(boxes)
    n = len(blo)
    words = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
    n_nodes = len(words)
    order = np.asarray(order).astype(np.int64)
    last = np.asarray(last).astype(np.int64)
    assert order.shape == (n,) and last.shape == (n,), "order and last have one entry per primitive"
    assert np.array_equal(np.sort(order), np.arange(n)), "order is not a permutation of 0..n-1"
    fl = words.view(np.float32)
    with np.errstate(all="ignore"):
        c2 = blo + bhi

    def child(i, side):
        o = 8 * side
        return int(words[i, o + 3]), int(words[i, o + 7]), fl[i, o:o + 3], fl[i, o + 4:o + 7]

    wrapped = int(words[0, 11]) == EMPTY
    leaves = []                                                            # (first, count, depth, node, side)
    node_depth = {0: 0}
    refs = np.zeros(n_nodes, np.int64)
    if wrapped:
        assert n_nodes == 1, "an empty child outside a one-node tree"
        c, cnt, _, _ = child(0, 0)
        assert c == (LEAF | 0) and cnt == n, f"node 0: a wrapped root holds one leaf of all {n} primitives"
        assert int(words[0, 15]) == 0 and (fl[0, 8:11] == np.float32(3.0e38)).all() and (fl[0, 12:15] == np.float32(3.0e38)).all(), "node 0: the empty child's record"
        leaves.append((0, n, 0, 0, 0))
    else:
        for i in range(n_nodes):
            assert i in node_depth, f"node {i} is referenced by no node before it"
            for side in (0, 1):
                c, cnt, _, _ = child(i, side)
                assert c != EMPTY, f"node {i} child {side}: empty child in a tree that is not a wrapped root"
                if c & LEAF:
                    assert cnt >= 1, f"node {i} child {side}: an empty leaf"
                    leaves.append((c & 0x7FFFFFFF, cnt, node_depth[i] + 1, i, side))
                else:
                    assert i < c < n_nodes, f"node {i} child {side}: inner index {c} is not a later node"
                    assert cnt == 0, f"node {i} child {side}: an inner child with a count"
                    refs[c] += 1
                    assert refs[c] == 1, f"node {c} is referenced twice (again by node {i})"
                    node_depth[c] = node_depth[i] + 1
        assert (refs[1:] == 1).all() and refs[0] == 0, "every inner index 1..n_nodes-1 is referenced exactly once"
    # the leaves tile [0, n), ascend inside, and carry the marks
    at = 0
    marks = np.zeros(n, np.int64)
    for first, cnt, d, i, side in sorted(leaves):
        assert first == at, f"node {i} child {side}: leaf starts at slot {first}, the slots before it end at {at}"
        assert first + cnt <= n, f"node {i} child {side}: leaf runs past the last slot"
        assert (np.diff(order[first:first + cnt]) > 0).all(), f"node {i} child {side}: order does not ascend inside the leaf"
        marks[first + cnt - 1] = 1
        at = first + cnt
    assert at == n, f"the leaves cover {at} of {n} slots"
    assert np.array_equal(last, marks), f"last differs from the leaves' last slots at slots {np.flatnonzero(last != marks)[:8]}"
    # depth and leaf sizes
    deepest = max(d for _, _, d, _, _ in leaves)
    assert deepest == depth, f"the deepest leaf lies at {deepest}, depth says {depth}"
    assert depth <= max_depth, f"depth {depth} beyond the limit {max_depth}"
    for first, cnt, d, i, side in leaves:
        if cnt > 8 and d < max_depth:
            c = c2[order[first:first + cnt]]
            assert (c == c[0]).all(), f"node {i} child {side}: a leaf of {cnt} primitives above the depth limit whose centroids differ"
    # boxes, children before parents: the exact union of the primitive boxes below every child (min and max do not round)
    prims_below = {}

    def below(i, side):
        c, cnt, _, _ = child(i, side)
        if c & LEAF:
            f = c & 0x7FFFFFFF
            return order[f:f + cnt]
        return prims_below[c]

    all_lo, all_hi = _padded(blo.min(axis=0), bhi.max(axis=0), abs_pad)
    own = {0: (all_lo, all_hi)}                                            # the box a node's parent holds for it
    for i in range(n_nodes):
        for side in (0, 1):
            c, _, lo_, hi_ = child(i, side)
            if c != EMPTY and not (c & LEAF):
                own[c] = (lo_, hi_)
    for i in range(n_nodes - 1, -1, -1):
        sides = (0,) if wrapped else (0, 1)
        u = []
        for side in sides:
            p = below(i, side)
            u.append((blo[p].min(axis=0), bhi[p].max(axis=0)))
        prims_below[i] = np.concatenate([below(i, side) for side in sides])
        tight = [_padded(x[0], x[1], abs_pad) for x in u]
        for side in sides:
            _, _, lo_, hi_ = child(i, side)
            assert (lo_ <= tight[side][0]).all() and (hi_ >= tight[side][1]).all(), \
                f"node {i} child {side}: box {lo_} {hi_} does not contain the padded union {tight[side][0]} {tight[side][1]} of its primitives"
        if all((child(i, side)[2] == tight[side][0]).all() and (child(i, side)[3] == tight[side][1]).all() for side in sides):
            continue
        # not tight: only the two halves of a hash split, which carry the node's own box and hold the primitives by their hash bit
        d = node_depth[i]
        carried = all((child(i, side)[2] == own[i][0]).all() and (child(i, side)[3] == own[i][1]).all() for side in sides)
        by_bit = not wrapped and all((hash_bit(below(i, side), d) == side).all() for side in sides)
        assert carried and by_bit, f"node {i}: a child box is not the padded union of its primitives, and the node is no hash split"
    return True
