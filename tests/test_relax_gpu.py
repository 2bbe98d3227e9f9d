"""Relaxation in torsion space on the device (fd_nerf_scan, fd_relax_energy, fd_relax, structures.relax, bin/relax_backbones.py,
bin/sample.py --relax) against fd_nerf, the numpy statement (tests/relax_reference.py) and its own invariants.
Needs an MI355X:  pytest -m gpu"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import relax_reference as rx
from conftest import GOLDEN, REPO
from foldingdiff_amd import _binding, nerf, structures
from test_relax import IDX, NEGATED_CHAINS, NEGATED_ITERS, negated_angle_case, random_features

pytestmark = pytest.mark.gpu

P = _binding.ptr
N_ITER = 60
NAMES3 = ["phi", "psi", "omega"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def pad(chains, L=None, fill=0.0):
    lens = np.array([len(c) for c in chains], dtype=np.int32)
    out = np.full((len(chains), L or int(lens.max()), chains[0].shape[1]), fill, dtype=np.float32)
    for b, c in enumerate(chains):
        out[b, : len(c)] = c
    return out, lens


def build(entry, feats, lens, idx, center):
    B, L, F = feats.shape
    out = np.full((B, 3 * L, 3), -7.0)
    _binding.check(getattr(_binding.load(), entry)(0, P(feats), P(lens), B, L, F, P(np.ascontiguousarray(idx, dtype=np.int32)), center, P(out)))
    return out


def params(prm: rx.Params, F):
    p = _binding.FdRelaxParams()
    for k in range(9):
        p.feat_idx[k] = int(prm.feat_idx[k])
    for f in range(F):
        p.is_angle[f], p.move[f] = int(bool(prm.is_angle[f])), int(bool(prm.move[f]))
    p.clash_alpha, p.clash_margin, p.w_clash, p.w_tether = prm.alpha, prm.margin, prm.w_clash, prm.w_tether
    p.step0, p.grow, p.shrink, p.max_step = prm.step0, prm.grow, prm.shrink, prm.max_step
    return p


def packed(rst, lens):
    """fd_restraint_energy's packed layout from one (i, j, d0, tol, w) tuple or None per chain."""
    sets = [None if r is None else structures.Restraints(*r) for r in (rst or [None] * len(lens))]
    return structures.pack_restraints(sets, [int(n) for n in lens])


def hook(feats, lens, prm, anchor=None, fixed=None, rst=None):
    """fd_relax_energy -> (energies [B, 3], gnorm [B], G [B, L, F] starting at the sentinel -7)."""
    B, L, F = feats.shape
    e, gn, G = np.full((B, 3), -7.0), np.full(B, -7.0), np.full((B, L, F), -7.0)
    p = params(prm, F)
    _binding.check(_binding.load().fd_relax_energy(0, P(feats), P(anchor), P(lens), B, L, F, C.byref(p), P(fixed), *(P(a) for a in packed(rst, lens)),
                                                   P(e), P(gn), P(G)))
    return e, gn, G


def relax(feats, lens, prm, n_iter, anchor=None, fixed=None, rst=None, step=None, out_fill=-7.0):
    """fd_relax -> (feats_out, energies, trace, accepted, step); feats_out starts at ``out_fill``."""
    B, L, F = feats.shape
    out, e, acc = np.full((B, L, F), out_fill, dtype=np.float32), np.full((B, 3), -7.0), np.full(B, -7, dtype=np.int32)
    trace = np.full((n_iter + 1, B), -7.0)
    step = None if step is None else np.array(step, dtype=np.float64)
    p = params(prm, F)
    _binding.check(_binding.load().fd_relax(0, P(feats), P(anchor), P(lens), B, L, F, C.byref(p), P(fixed), *(P(a) for a in packed(rst, lens)), n_iter,
                                            P(step), P(out), P(e), P(trace), P(acc)))
    return out, e, trace, acc, step


# ---------------------------------------------------------------------------------- 1. fd_nerf_scan against fd_nerf
@pytest.mark.parametrize("F", [3, 6, 9])
def test_scan_against_the_serial_builder(gpu, F):
    """Lengths 1, 2, 3, 7, 85, 86 (258 atoms: the first chain with more than one atom per lane), 128 and 2048 in one batch,
    centred or not: per chain within 1e-9 of its extent of fd_nerf, equal padding zeros, equal bits on a second call, and a
    chain's bits the same alone and inside a batch of five."""
    rng = np.random.default_rng(40 + F)
    chains = [random_features(rng, n, F) for n in (1, 2, 3, 7, 85, 86, 128, 2048)]
    feats, lens = pad(chains)
    worst = 0.0
    for center in (0, 1):
        want = build("fd_nerf", feats, lens, IDX[F], center)
        got = build("fd_nerf_scan", feats, lens, IDX[F], center)
        assert np.array_equal(bits(got), bits(build("fd_nerf_scan", feats, lens, IDX[F], center)))
        plain = want if center == 0 else build("fd_nerf", feats, lens, IDX[F], 0)
        for b, n in enumerate(lens):
            gate = rx.scan_gate(plain[b, : 3 * n])
            err = np.abs(got[b, : 3 * n] - want[b, : 3 * n]).max()
            worst = max(worst, err / gate * 1e-9)
            assert err <= gate, (F, center, n, err, gate)
            assert (got[b, 3 * n:] == 0).all() and (want[b, 3 * n:] == 0).all()
    print(f"F={F}: fd_nerf_scan is within {worst:.2e} of the chain's extent of fd_nerf")
    five, lens5 = pad([chains[3], chains[4], chains[5], chains[6], chains[2]])
    alone, lens1 = pad([chains[5]])
    for center in (0, 1):
        assert np.array_equal(bits(build("fd_nerf_scan", five, lens5, IDX[F], center)[2, : 3 * 86]),
                              bits(build("fd_nerf_scan", alone, lens1, IDX[F], center)[0]))


# ---------------------------------------------------------------------------------- 2. fd_relax_energy against the statement
def test_energy_and_gradient_against_the_statement_on_the_devices_coordinates(gpu):
    """Three chains of six features in one call: 343 residues (1029 atoms: past one 1024-atom LDS tile and four blocks of
    lanes), 2 residues (no pair that can clash), and 40 residues with restraints, fixed rows and an anchor of its own; phi
    and psi move, omega and the bond angles do not.  Energies within 1e-12 relative, the gradient within 1e-9 of the chain's
    largest entry, zeros exactly where `move` and `fixed` say, rows beyond a length untouched."""
    F = 6
    rng = np.random.default_rng(5)
    chains = [random_features(rng, n, F) for n in (343, 2, 40)]
    feats, lens = pad(chains)
    anchor = feats.copy()
    anchor[2, :40] = (feats[2, :40] + 0.05 * rng.standard_normal((40, F))).astype(np.float32)
    fixed = np.zeros((3, 343), dtype=np.uint8)
    fixed[2, [0, 7, 8, 39]] = 1
    fixed[0, 100:110] = 1
    rst = [None, None, ([1, 4, 118], [100, 61, 7], [5.0, 40.0, 3.0], [0.0, 1.0, 0.5], [1.0, 0.5, 2.0])]
    prm = rx.Params(IDX[F], [True] * 6, [True, True, False, False, False, False], w_clash=0.8, w_tether=0.3)
    e, gn, G = hook(feats, lens, prm, anchor, fixed, rst)
    e2, gn2, G2 = hook(feats, lens, prm, anchor, fixed, rst)
    assert np.array_equal(bits(e), bits(e2)) and np.array_equal(bits(gn), bits(gn2)) and np.array_equal(bits(G), bits(G2))
    coords = build("fd_nerf_scan", feats, lens, IDX[F], 0)
    for b, n in enumerate(lens):
        e_want, g_want, gn_want, _ = rx.relax_energy(chains[b], anchor[b, :n], prm, fixed[b, :n], rst[b], coords=coords[b, : 3 * n])
        scale = max(np.abs(g_want).max(), 1e-300)
        err_e = [abs(a - w) / w if w else abs(a) for a, w in zip(e[b], e_want)]
        err_g = np.abs(G[b, :n] - g_want).max() / scale
        print(f"{n} residues: E = {e[b]}, relative error {max(err_e):.2e}; gradient {err_g:.2e} of its largest entry; |G| {gn[b]:.6g}")
        assert max(err_e) <= 1e-12 and err_g <= 1e-9 and abs(gn[b] - gn_want) <= 1e-9 * max(gn_want, 1.0)
        assert (G[b, :n, 2:] == 0).all() and (G[b, :n][fixed[b, :n] == 1] == 0).all() and (G[b, n:] == -7).all()
    assert e[0, 0] > 0 and e[1, 0] == 0 and e[2, 1] > 0 and e[2, 2] > 0 and e[0, 2] == 0 and e[0, 1] == 0
    assert (G[0, :343, :2] != 0).sum() > 600
    # a NULL anchor is the input itself
    e0, _, G0 = hook(feats, lens, prm, None, fixed, rst)
    e1, _, G1 = hook(feats, lens, prm, feats, fixed, rst)
    assert (e0[:, 2] == 0).all() and np.array_equal(bits(e0), bits(e1)) and np.array_equal(bits(G0), bits(G1))


# ---------------------------------------------------------------------------------- 3. fd_relax
@pytest.fixture(scope="module")
def descent():
    """The batch of six chains (tests/test_relax.py shows what the statement does with them), relaxed once for N_ITER
    iterations with nothing fixed and every torsion free.  Computed once; the tests leave it unchanged."""
    chains = rx.device_chains()
    feats, lens = pad(chains, fill=123.0)
    prm = rx.Params(rx.IDX3, [True] * 3, [True] * 3)
    return dict(chains=chains, feats=feats, lens=lens, prm=prm, run=relax(feats, lens, prm, N_ITER))


def test_descent_never_rises_and_clears_every_clash(gpu, descent):
    out, e, trace, acc, _ = descent["run"]
    feats, lens, prm = descent["feats"], descent["lens"], descent["prm"]
    assert (np.diff(trace, axis=0) <= 0).all() and (trace[0] > 0).all() and (acc >= 1).all() and (acc <= N_ITER).all()
    assert np.array_equal(bits(trace[-1]), bits((e[:, 0] + e[:, 1]) + e[:, 2]))
    relaxed = [out[b, :n] for b, n in enumerate(lens)]
    for b, n in enumerate(lens):
        assert (out[b, n:] == -7).all()                                      # rows beyond the length keep what they held
    # energy_out is the hook on feats_out, bit for bit (anchor: the input, as in the run)
    e_hook, _, _ = hook(pad(relaxed, fill=55.0)[0], lens, prm, anchor=feats)
    assert np.array_equal(bits(e), bits(e_hook))
    # the soft term at 0 means the integer rule finds nothing on the float32 backbone
    backbones = nerf.build_backbones(descent["chains"] + relaxed, NAMES3, center_coords=False, method="scan")
    counts = structures.count_clashes(backbones)
    print(f"clashing atoms {counts[:6].tolist()} -> {counts[6:].tolist()}; E {trace[0].round(3).tolist()} -> {trace[-1].tolist()}; accepted {acc.tolist()}")
    assert (e[:, 0] == 0).all() and (counts[6:] == 0).all() and (counts[:6] >= 3).all()
    change = [np.abs(rx.wrap64(r.astype(np.float64) - c.astype(np.float64))).max() for r, c in zip(relaxed, descent["chains"])]
    assert max(change) < 1.0, change


def test_descent_equals_its_iterations_chained(gpu, descent):
    """N_ITER calls with n_iter = 1 chained through feats_out, step_io and the input as anchor give the run's bits."""
    out, e, trace, acc, _ = descent["run"]
    feats, lens, prm = descent["feats"], descent["lens"], descent["prm"]
    cur, step, total = feats, np.full(6, prm.step0), np.zeros(6, dtype=np.int64)
    for it in range(1, N_ITER + 1):
        nxt, e1, tr1, a1, step = relax(cur, lens, prm, 1, anchor=feats, step=step, out_fill=123.0)
        assert np.array_equal(bits(tr1[1]), bits(trace[it])), it
        cur, total = nxt, total + a1
    for b, n in enumerate(lens):
        assert np.array_equal(bits(cur[b, :n]), bits(out[b, :n])), b
    assert np.array_equal(bits(e1), bits(e)) and np.array_equal(total, acc)
    _, _, _, _, step_whole = relax(feats, lens, prm, N_ITER, step=np.full(6, prm.step0))
    assert np.array_equal(bits(step), bits(step_whole))


def test_a_chain_relaxes_the_same_alone_and_in_the_batch(gpu, descent):
    out, e, trace, acc, _ = descent["run"]
    for b in (0, 2, 5):
        n = int(descent["lens"][b])
        o1, e1, t1, a1, _ = relax(descent["feats"][b: b + 1, :n].copy(), descent["lens"][b: b + 1], descent["prm"], N_ITER)
        assert np.array_equal(bits(o1[0]), bits(out[b, :n])) and np.array_equal(bits(e1[0]), bits(e[b]))
        assert np.array_equal(bits(t1[:, 0]), bits(trace[:, b])) and a1[0] == acc[b]


@pytest.mark.parametrize("h,max_step", [(0.01, 0.5), (5.0, 50.0)])
def test_one_iteration_against_the_statement(gpu, descent, h, max_step):
    """From the hook's G and norm the statement's trial is within 2e-6 rad of the device's, and the decision is the
    statement's wherever the two energies differ by more than 1e-9 of the state's.  h = 5 with max_step = 50 is a step that
    the statement refuses for most chains."""
    feats, lens = descent["feats"], descent["lens"]
    prm = descent["prm"]._replace(max_step=max_step)
    e0, gn, G = hook(feats, lens, prm)
    out, e1, trace, acc, step = relax(feats, lens, prm, 1, step=np.full(6, h))
    decided = 0
    for b, n in enumerate(lens):
        x = descent["chains"][b]
        xt = rx.trial(x, G[b, :n], gn[b], h, prm)
        E = (e0[b, 0] + e0[b, 1]) + e0[b, 2]
        e_t = rx.relax_energy(xt, x, prm)[0]
        Et = (e_t[0] + e_t[1]) + e_t[2]
        assert trace[0, b] == E
        if abs(Et - E) > 1e-9 * E:
            assert bool(acc[b]) == bool(Et <= E), (b, E, Et, acc[b])
            decided += 1
        want = xt if acc[b] else x
        assert np.abs(rx.wrap64(out[b, :n].astype(np.float64) - want.astype(np.float64))).max() <= 2e-6
        assert step[b] == h * (prm.grow if acc[b] else prm.shrink)
        if not acc[b]:
            assert np.array_equal(bits(out[b, :n]), bits(x)) and np.array_equal(bits(e1[b]), bits(e0[b]))
    print(f"h={h}: accepted {acc.tolist()}, {decided} decisions compared")
    assert decided >= 4 and ((acc == 0).any() if h > 1 else (acc == 1).all())


def test_fixed_rows_and_immovable_columns_keep_their_bits_and_a_tether_holds_back(gpu, descent):
    feats, lens, prm = descent["feats"], descent["lens"], descent["prm"]
    fixed = np.zeros(feats.shape[:2], dtype=np.uint8)
    for b, n in enumerate(lens):
        fixed[b, 2:6] = 1
        fixed[b, n - 1] = 1
    held = prm._replace(move=[True, True, False])
    out, e, trace, acc, _ = relax(feats, lens, held, 12, fixed=fixed, out_fill=-9.0)
    assert (np.diff(trace, axis=0) <= 0).all() and (trace[-1] < trace[0]).all()
    for b, n in enumerate(lens):
        rows = fixed[b, :n] == 1
        assert np.array_equal(bits(out[b, :n][rows]), bits(feats[b, :n][rows]))
        assert np.array_equal(bits(out[b, :n, 2]), bits(feats[b, :n, 2]))
        assert (out[b, n:] == -9).all() and not np.array_equal(bits(out[b, :n]), bits(feats[b, :n]))
    # with a tether no angle moves further than without
    change = lambda o: np.array([np.abs(rx.wrap64(o[b, :n].astype(np.float64) - feats[b, :n].astype(np.float64))).max()   # noqa: E731
                                 for b, n in enumerate(lens)])
    free = change(descent["run"][0])
    tied_out, tied_e, tied_trace, _, _ = relax(feats, lens, prm._replace(w_tether=5.0), N_ITER)
    tied = change(tied_out)
    print(f"largest angle change: free {free.round(3).tolist()}, tether 5: {tied.round(3).tolist()}")
    assert (tied <= free).all() and (np.diff(tied_trace, axis=0) <= 0).all() and (tied_e[:, 2] > 0).any()
    # n_iter = 0 returns the input and its energy
    same, e_same, tr0, acc0, _ = relax(feats, lens, prm, 0)
    for b, n in enumerate(lens):
        assert np.array_equal(bits(same[b, :n]), bits(feats[b, :n]))
    assert (acc0 == 0).all() and np.array_equal(bits(e_same), bits(hook(feats, lens, prm)[0])) and np.array_equal(bits(tr0[0]), bits(descent["run"][2][0]))


def test_descent_on_negated_bond_angles_needs_the_signed_derivative(gpu):
    """Backbone-like chains of 7, 12, 40 and 86 residues with every bond angle negated and its torsion moved by pi (the same
    chains), restraints only, only the three bond-angle columns free, 10 iterations: every chain accepts at least one step and
    ends below its start.  With the bond-angle gradient negated -- the derivative from the coordinates alone -- every trial
    rises and nothing is accepted: tests/test_relax.py shows on the CPU that the statement accepts 7, 7, 4 and 2 steps on these
    seeds and the unsigned one none.  The hook's gradient agrees with the statement on the device's coordinates within 1e-9 of
    the chain's largest entry, zero in the torsion columns."""
    cases = [negated_angle_case(n, seed) for n, seed in NEGATED_CHAINS]
    prm = cases[0][2]
    feats, lens = pad([c[0] for c in cases], fill=55.0)
    rst = [c[1] for c in cases]
    e, gn, G = hook(feats, lens, prm, rst=rst)
    coords = build("fd_nerf_scan", feats, lens, IDX[6], 0)
    for b, n in enumerate(lens):
        e_want, g_want, gn_want, _ = rx.relax_energy(cases[b][0], None, prm, None, rst[b], coords=coords[b, : 3 * n])
        assert np.abs(G[b, :n] - g_want).max() <= 1e-9 * np.abs(g_want).max() and abs(gn[b] - gn_want) <= 1e-9 * gn_want
        assert (G[b, :n, :3] == 0).all() and (G[b, : n - 1, 3:] != 0).all() and e[b, 0] == 0 and e[b, 2] == 0 and e[b, 1] > 0
    out, e_out, trace, acc, _ = relax(feats, lens, prm, NEGATED_ITERS, rst=rst)
    print(f"E {trace[0].round(3).tolist()} -> {trace[-1].round(3).tolist()}; accepted {acc.tolist()}")
    assert (acc >= 1).all() and (trace[-1] < trace[0]).all() and (np.diff(trace, axis=0) <= 0).all()
    for b, n in enumerate(lens):
        assert np.array_equal(bits(out[b, :n, :3]), bits(feats[b, :n, :3])) and (out[b, n:] == -7).all()


# ---------------------------------------------------------------------------------- 4. end to end
def test_relax_on_1crn(gpu):
    """structures.relax on 1CRN's featurised angles (six features: the backbone is rebuilt on ideal bond lengths) with
    tether = 1: the energy does not rise and the relaxed backbone superposes on the unrelaxed rebuild."""
    df = structures.featurize([os.path.join(GOLDEN, "1CRN.pdb")], distances=(), angles=structures.EXHAUSTIVE_ANGLES)[0]
    names = list(df.columns)
    angles = np.nan_to_num(df.values.astype(np.float32), nan=0.0)
    res = structures.relax([angles], None, names, tether=1.0, n_iter=50, return_trace=True)
    before, after = res.energy_before.sum(axis=1), res.energy_after.sum(axis=1)
    start, end = (nerf.build_backbones([a], names, center_coords=False, method="scan")[0] for a in (angles, res.angles[0]))
    rmsd = structures.superposed_rmsd([end], [start])[0]
    print(f"1CRN: E {before[0]:.4f} -> {after[0]:.4f}, clashing atoms {res.clashes_before[0]} -> {res.clashes_after[0]}, accepted "
          f"{res.accepted[0]}, largest angle change {res.max_change[0]:.4f} rad, RMSD to the unrelaxed rebuild {rmsd:.4f} A")
    assert after[0] <= before[0] and np.isfinite(rmsd) and (np.diff(res.trace[:, 0]) <= 0).all()
    assert res.trace[0, 0] == before[0] and res.trace[-1, 0] == after[0] and res.angles[0].shape == angles.shape
    e, gn, grad = structures.relax_energy([angles], None, names)
    assert np.array_equal(e, res.energy_before) and grad[0].shape == angles.shape and (grad[0][:, 3:] == 0).all()
    # a native backbone has nothing to repair at the default margin; with one wide enough to be active the descent has work
    wide = structures.relax([angles], None, names, tether=1.0, margin=1.0, n_iter=50)
    end_wide = nerf.build_backbones([wide.angles[0]], names, center_coords=False, method="scan")[0]
    print(f"1CRN, margin 1.0: E {wide.energy_before.sum():.3f} -> {wide.energy_after.sum():.3f}, accepted {wide.accepted[0]}, largest angle "
          f"change {wide.max_change[0]:.4f} rad, RMSD to the unrelaxed rebuild {structures.superposed_rmsd([end_wide], [start])[0]:.4f} A")
    assert wide.energy_before[0, 0] > 0 and wide.energy_after.sum() < wide.energy_before.sum() and wide.energy_after[0, 2] > 0


def test_relax_backbones_cli(gpu, tmp_path):
    """bin/relax_backbones.py on a folder of angle CSVs and on a PDB file: relaxed CSVs, PDB files and relax_report.json."""
    import pandas as pd
    src = tmp_path / "sampled_angles"
    os.makedirs(src)
    for i, c in enumerate(rx.device_chains()[:2]):
        pd.DataFrame(c, columns=NAMES3).to_csv(src / f"generated_{i}.csv.gz")
    cli = os.path.join(REPO, "bin", "relax_backbones.py")
    out = tmp_path / "relaxed"
    r = subprocess.run([sys.executable, cli, str(src), "-o", str(out), "--n_iter", "60"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["relax_report.json", "relaxed_angles", "relaxed_pdb"]
    report = json.load(open(out / "relax_report.json"))
    assert sorted(report["chains"]) == ["generated_0", "generated_1"]
    for name, row in report["chains"].items():
        assert sorted(row) == ["accepted", "clashes_after", "clashes_before", "energy_after", "energy_before", "max_angle_change"]
        assert row["clashes_after"] == 0 and row["clashes_before"] >= 3 and sum(row["energy_after"]) <= sum(row["energy_before"])
        assert os.path.getsize(out / "relaxed_pdb" / f"{name}.pdb") > 0
        got = pd.read_csv(out / "relaxed_angles" / f"{name}.csv.gz", index_col=0)
        assert list(got.columns) == NAMES3 and len(got) == (12 if name == "generated_0" else 40)
    out2 = tmp_path / "relaxed_pdb_input"
    r = subprocess.run([sys.executable, cli, "--pdb", os.path.join(GOLDEN, "1CRN.pdb"), "-o", str(out2), "--n_iter", "5", "--tether", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert list(json.load(open(out2 / "relax_report.json"))["chains"]) == ["1CRN"] and os.path.exists(out2 / "relaxed_pdb" / "1CRN.pdb")


def test_sample_cli_relax(gpu, tmp_path):
    """bin/sample.py --relax N on a toy model: the usual tree plus relaxed_angles, relaxed_pdb and relax_report.json."""
    from test_clash_lddt_gpu import _mini_model_dir
    mdir = _mini_model_dir(tmp_path)
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "sample.py"), "-m", mdir, "-o", out, "-n", "2", "-l", "9", "12",
                        "-b", "4", "--seed", "3", "--relax", "20"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["model_snapshot", "relax_report.json", "relaxed_angles", "relaxed_pdb", "sampled_angles", "sampled_pdb"]
    report = json.load(open(os.path.join(out, "relax_report.json")))["chains"]
    assert list(report) == [f"generated_{i}" for i in range(6)]
    assert all(sum(row["energy_after"]) <= sum(row["energy_before"]) for row in report.values())
    assert sorted(os.listdir(os.path.join(out, "relaxed_pdb"))) == sorted(f"generated_{i}.pdb" for i in range(6))
