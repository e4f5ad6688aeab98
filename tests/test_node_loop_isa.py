"""The node loops of the persistent kernels' walkers, read from the compiler's assembly (rtamd_api.hip for gfx950 with the Makefile's flags, one
compile, no GPU): a node step writes no walk state but `cur`, `sp`, `steps` and the parked leaves (rt_persistent.h pt_walk_stint), so the loops
carry no copies of the rest.  Asserted: the budget of the four plain kernels, no flat access, and for the three hw8 / hw7 kernels both node
loops below the parent's VALU counts at once.  The parent (commit 548de05, profiles/r39_node_loops.txt) had 183 VALU in the closest-hit node loop
and 124 in the light node loop between the loop's top and its last branch back, as tests/test_walker_loads_isa.py finds them.  A loop is
counted here in two ways and the bound holds for both: between its first and last line as that file's helpers find it, and as every block
that the compiler's own loop annotation (`Header=`) assigns to it, which also holds blocks laid out after the last branch back (the parent:
167 and 132 that way).  The loops are told apart by content: the closest-hit loop sorts its children (v_min_u32 / v_max_u32).
v_mov counts are printed, not asserted."""
import re

import pytest

from test_walker_loads_isa import KERNELS, PT_KERNELS, _hot_loops, _insn, compiled  # noqa: F401  (compiled: the module-scoped fixture, one compile for this file)

PARENT_VALU = {"closest-hit": 183, "light": 124}  # the parent's node loops, pt_persistent_kernel<false,0|1|2> alike


def _by_header(body, a, b):
    """instructions of every block that the assembly's loop annotation assigns to the loop whose lines a..b hold its header"""
    hdr = next((m.group(1) for l in body[a:b + 1] for m in [re.search(r"Header=(BB\d+_\d+) ", l)] if m), None)
    out, on = [], False
    for l in body:
        m = re.match(r"^\.L(BB\d+_\d+):(.*)", l)
        if m:
            on = hdr is not None and (m.group(1) == hdr or f"Header={hdr} " in m.group(2))
        elif on and _insn(l):
            out.append(_insn(l))
    return out


def _stats(ins):
    return {"all": len(ins), "VALU": sum(x.startswith("v_") for x in ins), "v_mov": sum(x.startswith("v_mov_b") for x in ins),
            "v_readlane": sum(x.startswith("v_readlane") for x in ins), "SALU": sum(x.startswith("s_") for x in ins)}


def _loops(body):
    """{'closest-hit' | 'light': {'node': (range stats, header stats), 'leaf': ...}}"""
    nodes, leaves = _hot_loops(body)
    assert len(nodes) == 2 and len(leaves) == 2
    out = {}
    for (a, b), (c, d) in zip(nodes, leaves):
        ins = [x for x in map(_insn, body[a:b + 1]) if x]
        sorts = sum(x.startswith(("v_min_u32", "v_max_u32")) for x in ins)
        role = "closest-hit" if sorts else "light"
        assert role not in out
        out[role] = {"node": (_stats(ins), _stats(_by_header(body, a, b))),
                     "leaf": (_stats([x for x in map(_insn, body[c:d + 1]) if x]), _stats(_by_header(body, c, d)))}
    assert sorted(out) == ["closest-hit", "light"]
    return out


def test_budget_and_no_flat_access(compiled):
    bodies, usage = compiled
    for k in KERNELS:
        print(k, usage[k])
        assert not [l for l in bodies[k] if (_insn(l) or "").startswith("flat_")], k
        u = usage[k]
        assert u["VGPRs"] <= 96 and u["ScratchSize"] == 0 and u["Occupancy"] == 5 and u["LDS Size"] <= 32000, (k, u)


@pytest.mark.parametrize("kernel", PT_KERNELS)
def test_both_node_loops_below_the_parents(compiled, kernel):
    loops = _loops(compiled[0][kernel])
    for role in ("closest-hit", "light"):
        for part in ("node", "leaf"):
            print(f"{kernel} {role} {part} loop: first to last line {loops[role][part][0]}, by header {loops[role][part][1]}")
    for role, bound in PARENT_VALU.items():  # both at once
        by_range, by_header = loops[role]["node"]
        assert by_range["VALU"] < bound and by_header["VALU"] < bound, (kernel, role, by_range, by_header)


def test_hw6_loops_are_reported(compiled):
    """p6_persistent_kernel<false> shares the loop (immediate endings): its four loops for the record, no bound."""
    body = compiled[0]["p6_persistent_kernelILb0EEE"]
    nodes, leaves = _hot_loops(body)
    for kind, found in (("node", nodes), ("leaf", leaves)):
        for a, b in found:
            print(f"hw6 {kind} loop, lines {a}-{b}: {_stats([x for x in map(_insn, body[a:b + 1]) if x])}, by header {_stats(_by_header(body, a, b))}")
    assert len(nodes) == 2
