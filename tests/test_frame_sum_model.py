"""The frame walk of csrc/device/rt_ref_walk.h (FrameWalk, frame_sum) as a plain-Python model of ONE frame_sum call: the stack, the tag
words and the two moves, with float32 additions.  The model is the specification: it is held here to the obvious recursion
total(node) = total(left) + total(right), and test_gpu_frame_sum.py holds the device function to it bit for bit.

A tree is a table of nodes (kind, left, right, value): TOTAL — this side's total is `value` (a leaf's sum, a failed box, or 0);
ONE — only `left` can contribute, no frame; BOTH — total(left) + total(right), `right` waits on the stack.  A BOTH met with MAXDEPTH
frames on the stack counts as a total of 0 (the hosts refuse such trees; the model says what happens anyway)."""
import numpy as np

TOTAL, ONE, BOTH = 0, 1, 2
f32 = np.float32


def bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def unbits(w):
    return np.array([w], np.uint32).view(np.float32)[0]


def frame_sum_model(nodes, root, maxdepth):
    """One frame_sum<maxdepth> call on the tree under `root`; returns the float32 total."""
    words = (maxdepth + 63) // 64
    add = [0] * words                 # frame kind per stack slot: 1 = ADD(partial sum), 0 = TODO(child)
    stack = [0] * maxdepth            # words: a node number (TODO) or the bits of a float32 (ADD)
    sp, v, cur, descending = 0, f32(0), root, True

    def tag(i, is_add):
        if is_add:
            add[i >> 6] |= 1 << (i & 63)
        else:
            add[i >> 6] &= ~(1 << (i & 63))

    while True:
        if descending:                # down(kind, l, r)
            kind, l, r, value = nodes[cur]
            if kind == BOTH and sp >= maxdepth:
                kind, value = TOTAL, f32(0)
            if kind == TOTAL:
                v, descending = f32(value), False
            else:
                if kind == BOTH:
                    tag(sp, False)
                    stack[sp] = r
                    sp += 1
                cur = l
        else:                         # up()
            if sp == 0:
                return v
            sp -= 1
            f = stack[sp]
            if (add[sp >> 6] >> (sp & 63)) & 1:
                v = f32(unbits(f) + v)          # left total + right total
            else:
                tag(sp, True)
                stack[sp] = bits(v)
                sp += 1
                cur, descending = f, True


def recursion(nodes, node, maxdepth, sp=0):
    """FiguresMix::getTotalPdf as the reference writes it, with the depth rule of the model (sp: frames on the stack at this node)."""
    kind, l, r, value = nodes[node]
    if kind == TOTAL:
        return f32(value)
    if kind == ONE:
        return recursion(nodes, l, maxdepth, sp)
    if sp >= maxdepth:
        return f32(0)
    return f32(recursion(nodes, l, maxdepth, sp + 1) + recursion(nodes, r, maxdepth, sp + 1))


def leaves_in_order(nodes, node):
    kind, l, r, value = nodes[node]
    if kind == TOTAL:
        return [f32(value)]
    if kind == ONE:
        return leaves_in_order(nodes, l)
    return leaves_in_order(nodes, l) + leaves_in_order(nodes, r)


def leaf_value(rng):
    """mixed magnitudes u * 2^e, e in [-12, 12]; a quarter of the leaves are zeros (a miss, a failed box); no term is negative"""
    if rng.random() < 0.25:
        return f32(0)
    return f32(np.ldexp(f32(rng.random()), int(rng.integers(-12, 13))))


def random_tree(rng, nodes, n_leaves):
    """appends a random tree of n_leaves leaves to the table, returns its root"""
    if n_leaves == 1:
        nodes.append((TOTAL, 0, 0, leaf_value(rng)))
    else:
        k = int(rng.integers(1, n_leaves))
        l = random_tree(rng, nodes, k)
        r = random_tree(rng, nodes, n_leaves - k)
        nodes.append((BOTH, l, r, f32(0)))
    if rng.random() < 0.2:            # all hits on one side: the walk goes on there without a frame
        nodes.append((ONE, len(nodes) - 1, 0, f32(0)))
    return len(nodes) - 1


def random_forest(seed, n_trees, max_leaves=40, min_leaves=1):
    rng = np.random.default_rng(seed)
    nodes, roots = [], []
    for _ in range(n_trees):
        roots.append(random_tree(rng, nodes, int(rng.integers(min_leaves, max_leaves + 1))))
    return nodes, roots


def chain(rng, nodes, depth, left_deep):
    """`depth` nested BOTH nodes, the next one always on the same side: the stack grows to `depth` frames"""
    nodes.append((TOTAL, 0, 0, leaf_value(rng)))
    inner = len(nodes) - 1
    for _ in range(depth):
        nodes.append((TOTAL, 0, 0, leaf_value(rng)))
        leaf = len(nodes) - 1
        nodes.append((BOTH, inner, leaf, f32(0)) if left_deep else (BOTH, leaf, inner, f32(0)))
        inner = len(nodes) - 1
    return inner


def chains(seed, maxdepth):
    """left-deep and right-deep chains of depth maxdepth - 1, maxdepth and maxdepth + 1 (the last meets the depth rule)"""
    rng = np.random.default_rng(seed)
    nodes, roots = [], []
    for depth in (maxdepth - 1, maxdepth, maxdepth + 1):
        for left_deep in (True, False):
            roots.append(chain(rng, nodes, depth, left_deep))
    return nodes, roots


def test_the_model_is_the_recursion_on_random_trees():
    nodes, roots = random_forest(11, 400)
    kinds = {k for k, _, _, _ in nodes}
    assert kinds == {TOTAL, ONE, BOTH}
    for maxdepth in (64, 128):
        for root in roots:
            got, want = frame_sum_model(nodes, root, maxdepth), recursion(nodes, root, maxdepth)
            assert bits(got) == bits(want), (root, got, want)


def test_the_association_matters_on_these_trees():
    """A walk that added the same leaves in another association (left to right, say) must not pass: on at least half of the trees with
    three or more non-zero leaves the reference's association gives another float32 than the running sum.  Trees of 3 to 100 leaves (a
    scene's light tree holds hundreds of lights): how often the association shows grows with the number of additions, from 48 % of the
    trees of up to 40 leaves to 67 % of these; half is asked of a set that leaves that room."""
    nodes, roots = random_forest(11, 400, 100, 3)
    judged = differ = 0
    for root in roots:
        leaves = leaves_in_order(nodes, root)
        if sum(1 for x in leaves if x != 0) < 3:
            continue
        running = f32(0)
        for x in leaves:
            running = f32(running + x)
        judged += 1
        differ += bits(running) != bits(frame_sum_model(nodes, root, 64))
    print(f"{differ} of {judged} trees with three or more non-zero leaves differ from the left-to-right sum")
    assert judged >= 300 and 2 * differ >= judged


def test_chains_fill_the_stack_and_meet_the_depth_rule():
    for maxdepth in (64, 128):
        nodes, roots = chains(3, maxdepth)
        for i, root in enumerate(roots):
            depth = maxdepth - 1 + i // 2
            got = frame_sum_model(nodes, root, maxdepth)
            assert bits(got) == bits(recursion(nodes, root, maxdepth)), (maxdepth, depth)
            unlimited = recursion(nodes, root, 1 << 30)
            if depth <= maxdepth:
                assert bits(got) == bits(unlimited)
    # the rule itself: the innermost BOTH of a chain one too deep counts as 0, so its two leaves drop out of the sum
    nodes = []
    rng = np.random.default_rng(5)
    root = chain(rng, nodes, 65, True)
    cut = [(TOTAL, 0, 0, f32(0)) if i == 2 else n for i, n in enumerate(nodes)]   # node 2 is the innermost BOTH
    assert nodes[2][0] == BOTH
    assert bits(frame_sum_model(nodes, root, 64)) == bits(recursion(cut, root, 1 << 30))
