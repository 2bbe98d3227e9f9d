"""The conditions the call-history tests rest on (tests/call_history_cases.py), checked without a device: the lengths of any
two kinds move some sequence down and some up, the moves include the edges the kernels have, and the shape-cache schedule
produces the parked return, the evictions and the returns it claims under a restatement of ensure_ws's policy."""
import itertools

import call_history_cases as cases


def test_every_kind_has_its_own_permutation_of_the_lengths():
    seen = {}
    for kind in cases.A_KINDS:
        lens = cases.lens_of(kind)
        if kind == "steered":     # one group of five particles: one length, inside the range of the others and with their 320 rows
            assert lens == (cases.STEERED_LEN,) * cases.B and min(cases.LENGTHS) < cases.STEERED_LEN < max(cases.LENGTHS)
            assert cases.STEERED_LEN in cases.LENGTHS and cases.B * cases.ceil8(cases.STEERED_LEN) == 320
        else:
            assert sorted(lens) == sorted(cases.LENGTHS), kind
        assert lens not in seen, (kind, seen.get(lens))
        seen[lens] = kind
    assert set(cases.B_KINDS) < set(cases.A_KINDS) and set(cases.A_KINDS) - set(cases.B_KINDS) == {"run_left_open", "refused"}
    assert len(cases.A_KINDS) == 25 and len(cases.B_KINDS) == 23
    # the kinds that were there first keep their place, and with it their lengths
    assert cases.A_KINDS[:18] == ("forward", "forward_t", "forward_ex", "step", "step_inpaint", "step_coef", "run_history", "run_packed",
                                  "run_host_noise", "inpaint", "inpaint_resample", "strided", "strided_inpaint_resample", "ar_forward",
                                  "ar_sample", "loss_ex", "run_left_open", "refused")
    assert cases.LATER_KINDS == ("solver", "strided_inpaint", "steered", "repeat", "step_coef_inpaint", "step_solver", "step_coef_x0")
    assert set(cases.LATER_PLANS) < set(cases.PLANS)
    for plan in cases.PLANS:
        got = cases.kinds_under(plan, cases.B_KINDS)
        assert got == (cases.B_KINDS if plan in cases.LATER_PLANS else cases.B_KINDS[:16]), plan
    for n, (start, period, units) in zip(cases.lens_of("repeat"), cases.repeat_ties(cases.lens_of("repeat"))):
        assert start >= 0 and period >= 1 and units >= 2 and start + period * units <= n, (n, start, period, units)
    for reduced in (cases.WIDE_KINDS, cases.ABS_KINDS, cases.F32_REFUSED):
        assert set(reduced) <= set(cases.B_KINDS)
    assert max(cases.LENGTHS) == cases.L <= 128 and max(cases.LENGTHS) < cases.T     # (fd_ar_*: seq_lengths < T)
    assert sum(cases.ceil8(n) for n in cases.LENGTHS) == 320                          # three 128-row passes, the last one part full
    starts = list(itertools.accumulate(cases.ceil8(n) for n in cases.lens_of("run_packed")))
    assert any(s % 128 for s in starts[:-1])                                          # pass borders inside sequences


def test_any_ordered_pair_of_kinds_moves_sequences_both_ways():
    for a, b in itertools.permutations(cases.A_KINDS, 2):
        tr = cases.transitions(cases.lens_of(a), cases.lens_of(b))
        assert tr["shorter"] and tr["longer"], (a, b)


def test_the_pairs_include_every_edge_for_every_first_kind():
    """Not every pair can cross every edge (the 7 has five places only); every first kind A meets each edge with some
    second kind, and every second kind B with some first kind: a change of ceil8 downwards and upwards, a sequence falling
    back into its first 32-key tile, a sequence crossing 96 in either direction."""
    edges = ("rows_shrink", "rows_grow", "leaves_tile", "leaves_96", "enters_96")
    count = dict.fromkeys(edges, 0)
    for a in cases.A_KINDS:
        met = set()
        for b in cases.B_KINDS:
            if a != b:
                tr = cases.transitions(cases.lens_of(a), cases.lens_of(b))
                met |= {e for e in edges if tr[e]}
                for e in edges:
                    count[e] += tr[e]
        # (five equal lengths cannot cross every edge: "steered" crosses the ones call_history_cases.STEERED_EDGES names)
        assert met == set(cases.STEERED_EDGES["first"] if a == "steered" else edges), (a, set(edges) - met)
    for b in cases.B_KINDS:
        met = set()
        for a in cases.A_KINDS:
            if a != b:
                tr = cases.transitions(cases.lens_of(a), cases.lens_of(b))
                met |= {e for e in edges if tr[e]}
        assert met == set(cases.STEERED_EDGES["second"] if b == "steered" else edges), (b, set(edges) - met)
    n_pairs = len(cases.A_KINDS) * len(cases.B_KINDS) - len(cases.B_KINDS)
    assert all(c >= n_pairs // 2 for c in count.values()), (count, n_pairs)     # and most pairs do


def test_group_e_lengths():
    b, pos, f = cases.POISON_AT
    assert pos >= 40 and pos < cases.POISON_LENS[b] and 0 <= f < cases.F
    assert min(cases.POISON_LENS) > 96 and max(cases.POISON_LENS) == cases.L
    assert cases.HEALTHY_PACKED_LENS[b] == 33 and sorted(cases.HEALTHY_PACKED_LENS) == sorted(cases.LENGTHS)
    # the poisoned position lies in a key tile the short sequence still reads (keys 32 .. 63 of a 33-long sequence) ...
    assert 32 <= pos < 64
    # ... behind the rows a packed run rewrites for it
    assert pos >= cases.ceil8(cases.HEALTHY_PACKED_LENS[b])


def test_cache_schedule_does_what_it_claims():
    events = cases.simulate_cache(cases.CACHE_SCHEDULE)
    assert len(events) == len(cases.CACHE_SCHEDULE)
    for step, claim in cases.CACHE_CLAIMS.items():
        assert claim in events[step], (step, claim, events[step])
    # the evicted shapes of the claims are the ones named in the comments
    assert cases.CACHE_SCHEDULE[6][0] == 1 and cases.CACHE_SCHEDULE[7][0] == 0
    everything = set().union(*events)
    assert {"parked_return", "parked_return_graph", "evict", "evict_graph", "recreate", "recreate_graph"} <= everything
    # every shape at least twice, never with the same lengths
    visits = {}
    for shape, _ in cases.CACHE_SCHEDULE:
        visits[shape] = visits.get(shape, 0) + 1
    assert set(visits) == set(range(len(cases.SHAPES))) and min(visits.values()) >= 2
    for shape, n in visits.items():
        b, l = cases.SHAPES[shape]
        lens = [cases.shape_lens(shape, v) for v in range(n)]
        assert len(set(lens)) == n, (shape, lens)
        assert all(len(x) == b and max(x) <= l and min(x) >= 1 for x in lens) and max(lens[0]) == l, (shape, lens)
    # at most four workspaces are ever alive: never more than three evictions pending, and the policy evicts before it allocates
    assert sum("evict" in e or "evict_graph" in e for e in events) >= 4


def test_the_restated_policy_on_a_hand_worked_sequence():
    """Shapes a b c d e a c a.  When d comes, c is parked as the third: a (the oldest stamp, with its graph) goes before d is
    made.  e: b goes.  a again: c goes, a is made anew.  c again: d goes, c is made anew.  a: still parked, a return without a
    graph (the new a only ran a forward)."""
    ev = cases.simulate_cache([("a", "run"), ("b", "forward"), ("c", "forward"), ("d", "forward"), ("e", "forward"), ("a", "forward"),
                               ("c", "forward"), ("a", "forward")])
    assert ev[:3] == [set(), set(), set()]
    assert ev[3] == {"evict_graph"}
    assert ev[4] == {"evict"}
    assert ev[5] == {"evict", "recreate_graph"}
    assert ev[6] == {"evict", "recreate"}
    assert ev[7] == {"parked_return"}


def test_option_states():
    assert cases.OPTION_STATES[0] == {"fuse_ffn": 2}
    for i in cases.OPTION_FLIPS_BACK:
        assert cases.OPTION_STATES[i] == cases.OPTION_STATES[0]
    assert all(set(s) <= set(cases.OPTION_DEFAULTS) for s in cases.OPTION_STATES)
    assert all(a != b for a, b in zip(cases.OPTION_STATES, cases.OPTION_STATES[1:]))    # every step changes something
    assert cases.OPTION_STATES[3]["rows_hint"] == 320
    assert set(cases.PLANS) == {"auto", "attn1_ffn2", "attn2_ffn1", "unfused", "attn1_ffn2_grid2"}
