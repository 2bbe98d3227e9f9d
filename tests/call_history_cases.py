"""
The call kinds and the schedules of the call-history tests (tests/test_call_history.py checks the conditions stated here on
the CPU; tests/test_call_history_gpu.py runs them).  Plain data and pure Python: no device, no torch.

A model handle keeps state between calls ("What a handle carries between calls").  The tests make a call B
after a call A on one handle and compare B's result BIT FOR BIT with the same call made first on a fresh handle.  So that a
stale row table, a stale key / value slot or a stale graph can show, every kind has its own lengths: a distinct permutation
of LENGTHS.  Two different permutations of the same numbers differ somewhere upwards and somewhere downwards, so for any
ordered pair of kinds some sequence gets shorter and some gets longer.  (One kind, "steered", cannot have a permutation: its
particles share a length.  What it keeps of the rule is stated at STEERED_LEN.)
"""
import itertools

B, L, F = 5, 101, 6
T = 130            # timesteps of the schedule: the autoregressive entries index the same table with a length < T
T_START = 3        # every run is t = 3, 2, 1, 0
# 101 and 97 lie beyond the 96 positions of the 16-row fused attention's three key tiles, 33 and 7 on either side of one
# 32-key tile, 7 below the 8-row packing; ceil8 = 104, 104, 64, 40, 8: 320 packed rows, three 128-row passes whose borders
# fall inside sequences
LENGTHS = (101, 97, 64, 33, 7)

# (name, may come second)
KINDS = (
    ("forward", True),                      # fd_forward
    ("forward_t", True),                    # fd_forward_t, mixed timesteps
    ("forward_ex", True),                   # fd_forward_ex, a mask with holes (absolute positions: explicit position_ids)
    ("step", True),                         # fd_p_sample_step
    ("step_inpaint", True),                 # fd_p_sample_step_inpaint
    ("step_coef", True),                    # fd_p_sample_step_coef
    ("run_history", True),                  # fd_sample: padded, Philox, every state, through the graph
    ("run_packed", True),                   # fd_sample: varlen = 1, final state only, through the graph
    ("run_host_noise", True),               # fd_sample: the caller's draws, use_graph = 0, every second state
    ("inpaint", True),                      # fd_sample_inpaint
    ("inpaint_resample", True),             # fd_sample_inpaint_resample, one jump
    ("strided", True),                      # fd_sample_strided, eta = 1
    ("strided_inpaint_resample", True),     # fd_sample_strided_inpaint_resample
    ("ar_forward", True),                   # fd_ar_forward
    ("ar_sample", True),                    # fd_ar_sample
    ("loss_ex", True),                      # fd_denoise_loss_ex with the pairwise term
    ("run_left_open", False),               # fd_sample_begin_dev + two steps, never ended
    ("refused", False),                     # calls refused for an argument error
    # the run families and step hooks that came later (appended: lens_of goes by index, the kinds above keep their lengths).
    # Their grids are the three visits 3, 1, 0 of "strided"
    ("solver", True),                       # fd_sample_solver, every state
    ("strided_inpaint", True),              # fd_sample_strided_inpaint, no jumps, the caller's known_noise, every state
    ("steered", True),                      # fd_sample_steered, two events, ONE group of five particles (see lens_of)
    ("repeat", True),                       # fd_sample_repeat, the caller's draws
    ("step_coef_inpaint", True),            # fd_p_sample_step_coef_inpaint
    ("step_solver", True),                  # fd_p_sample_step_solver, c != 0
    ("step_coef_x0", True),                 # fd_p_sample_step_coef_x0
)
A_KINDS = tuple(k for k, _ in KINDS)
B_KINDS = tuple(k for k, second in KINDS if second)
LATER_KINDS = A_KINDS[A_KINDS.index("refused") + 1:]
# The matrix of 25 x 23 kinds makes twice the calls of the 18 x 16 it was, so the later kinds run under three of the five plans
# (DESIGN.md 2): the default, both fusions off, and several items per workgroup
LATER_PLANS = ("auto", "unfused", "attn1_ffn2_grid2")

_PERMS = sorted(itertools.permutations(LENGTHS))
# fd_sample_steered wants one length per particle group, and B = 5 is one group of five or five groups of one (no steering): the
# kind stays on the (5, 101) workspace every other kind uses, with all five lengths at 64 -- 5 * 64 = 320 packed rows like the
# others.  Against any permutation of LENGTHS some sequence still gets shorter and some longer, either way round; of the five
# edges it cannot cross leaves_96 as a first call, nor leaves_tile and enters_96 as a second (STEERED_EDGES)
STEERED_LEN = 64
STEERED_EDGES = {"first": ("rows_shrink", "rows_grow", "leaves_tile", "enters_96"), "second": ("rows_shrink", "rows_grow", "leaves_96")}


def lens_of(kind: str) -> tuple:
    """The kind's lengths: permutation 7 i (mod 120) of the sorted list, i = the kind's index (7 and 120 are coprime); the
    one exception is "steered", whose five particles share STEERED_LEN."""
    if kind == "steered":
        return (STEERED_LEN,) * B
    return _PERMS[(7 * A_KINDS.index(kind)) % len(_PERMS)]


def kinds_under(plan: str, kinds: tuple) -> tuple:
    """`kinds` without the later ones under a plan that does not run them."""
    return tuple(k for k in kinds if plan in LATER_PLANS or k not in LATER_KINDS)


def repeat_ties(lens) -> tuple:
    """(start, period, units) per sequence of the "repeat" kind: three units behind a lead-in row, whatever the length
    (7: rows 1 .. 6 in units of 2; 101: rows 1 .. 99 in units of 33)."""
    return tuple((1, (n - 1) // 3, 3) for n in lens)


# the reduced matrices of the other models
WIDE_KINDS = ("forward", "forward_t", "forward_ex", "run_history", "run_packed", "run_host_noise", "inpaint", "inpaint_resample",
              "strided", "strided_inpaint_resample")
ABS_KINDS = ("forward", "forward_ex", "run_history", "ar_forward")
F32_REFUSED = ("forward_ex", "ar_forward", "ar_sample")      # FD_E_UNSUPPORTED on an FD_PREC_F32 model (include/fdmi.h)

# the launch plan, set once per handle
PLANS = {
    "auto": {},
    "attn1_ffn2": {"fuse_attn": 1, "fuse_ffn": 2},
    "attn2_ffn1": {"fuse_attn": 2, "fuse_ffn": 1},
    "unfused": {"fuse_attn": 0, "fuse_ffn": 0},
    "attn1_ffn2_grid2": {"fuse_attn": 1, "fuse_ffn": 2, "debug_grid": 2},   # several items per workgroup meet the stale state
}


def ceil8(n: int) -> int:
    return (n + 7) // 8 * 8


def transitions(a: tuple, b: tuple) -> dict:
    """What happens to the sequences when lengths b follow lengths a on one workspace."""
    pairs = list(zip(a, b))
    return {
        "shorter": any(y < x for x, y in pairs),
        "longer": any(y > x for x, y in pairs),
        "rows_shrink": any(ceil8(y) < ceil8(x) for x, y in pairs),      # packed rows of a sequence go away
        "rows_grow": any(ceil8(y) > ceil8(x) for x, y in pairs),
        "leaves_tile": any(x > 32 >= y for x, y in pairs),              # a sequence falls back into its first 32-key tile
        "leaves_96": any(x > 96 >= y for x, y in pairs),                # ... back into the 16-row fused attention's range
        "enters_96": any(y > 96 >= x for x, y in pairs),
    }


# ---- the shape cache (group B).  ensure_ws keeps the current workspace and up to three parked ones.
SHAPES = ((5, 101), (3, 128), (7, 33), (2, 16), (4, 64), (1, 7))
# (shape index, call): "run" = a padded run through the graph (captures one), "packed" = a packed run through the graph,
# "forward" / "step" = no graph.  The visit number of a shape picks its lengths (shape_lens).
CACHE_SCHEDULE = (
    (0, "run"), (1, "forward"), (0, "run"), (2, "packed"), (3, "forward"), (4, "step"), (1, "step"), (0, "packed"), (5, "forward"),
    (2, "run"), (3, "step"), (4, "run"), (5, "run"), (0, "forward"), (1, "run"), (3, "forward"), (1, "packed"),
    (3, "step"),
)
# what the schedule claims, by step index (checked against simulate_cache on the CPU)
CACHE_CLAIMS = {
    2: "parked_return_graph",      # back to a parked shape that holds a captured graph
    4: "evict",                    # the least recently used shape goes (shape 1, no graph)
    5: "evict_graph",              # a shape whose graph was captured goes (shape 0)
    6: "recreate",                 # back to the evicted shape 1
    7: "recreate_graph",           # back to shape 0, whose graph went with it
}


def shape_lens(shape: int, visit: int) -> tuple:
    """Lengths of the visit-th call on a shape: one full-length sequence (another one each visit; a batch of one is full
    length on its even visits only), the others spread over 1 .. L; no two visits of a shape agree."""
    b, l = SHAPES[shape]
    out = [1 + ((7 * i + 13 * visit + 3) * 11) % l for i in range(b)]
    if b > 1 or visit % 2 == 0:
        out[visit % b] = l
    return tuple(out)


def simulate_cache(schedule) -> list:
    """ensure_ws's policy restated: the current workspace is stamped and parked, a parked one of the wanted shape is taken
    back, otherwise the oldest stamps go until at most two stay parked and a new (zeroed, graphless) one is made.
    Returns the set of events of every call."""
    cur, parked, clock, gone, events = None, [], 0, {}, []
    for shape, call in schedule:
        clock += 1
        ev = set()
        if cur is not None:
            cur["stamp"] = clock
        if cur is None or cur["shape"] != shape:
            if cur is not None:
                parked.append(cur)
            hit = [w for w in parked if w["shape"] == shape]
            if hit:
                cur = hit[0]
                parked.remove(cur)
                ev.add("parked_return_graph" if cur["graph"] else "parked_return")
            else:
                while len(parked) >= 3:
                    old = min(parked, key=lambda w: w["stamp"])
                    parked.remove(old)
                    gone[old["shape"]] = old["graph"]
                    ev.add("evict_graph" if old["graph"] else "evict")
                if shape in gone:
                    ev.add("recreate_graph" if gone.pop(shape) else "recreate")
                cur = {"shape": shape, "graph": False}
            cur["stamp"] = clock
        cur["graph"] = cur["graph"] or call in ("run", "packed")
        events.append(ev)
    return events


# ---- options changed while a workspace is parked, and on the current one (group C): the options in force, in order.
# Every state is compared with a fresh handle under the same options; the states named in OPTION_FLIPS_BACK return to state 0.
OPTION_STATES = (
    {"fuse_ffn": 2},
    {"fuse_ffn": 0},
    {"fuse_ffn": 2},
    {"fuse_ffn": 2, "varlen": 1, "rows_hint": sum(ceil8(n) for n in LENGTHS)},
    {"fuse_ffn": 2},
    {"fuse_ffn": 2, "fuse_attn": 0},
    {"fuse_ffn": 2, "fuse_attn": 1},
    {"fuse_ffn": 2, "fuse_attn": 0},
    {"fuse_ffn": 2},
)
OPTION_FLIPS_BACK = (2, 4, 8)
OPTION_DEFAULTS = {"fuse_ffn": -1, "fuse_attn": -1, "varlen": 0, "rows_hint": 0}

# ---- after a non-finite call (group E)
POISON_LENS = (101, 97, 101, 99, 98)       # the poisoned padded forward: long sequences
POISON_AT = (2, 57, 3)                     # (sequence, position, feature) of the NaN / Inf: valid, at or beyond position 40
HEALTHY_PACKED_LENS = (64, 101, 33, 7, 97)  # the packed run behind it: the poisoned sequence is 33 long
