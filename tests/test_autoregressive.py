"""
The autoregressive baseline without a GPU: the CPU restatement (tests/ar_reference.py) against the reference class's own
forward and rollout (tests/golden/ref_autoregressive.npz, written by make_golden_autoregressive.py), the argument checks
of ``modelling.BertForAutoregressiveBase``, the command line of bin/sample_autoregressive.py and the two C entries' checks.

GOLDEN_TOL 5e-6 is the gate test_oracle_golden.py holds the oracle to against the reference class.
"""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import ar_reference
from conftest import GOLDEN, REPO, golden
from foldingdiff_amd import _binding, modelling, structures
from oracle import ref_model

GOLDEN_TOL = 5e-6


def _cli():
    spec = importlib.util.spec_from_file_location("sample_autoregressive", os.path.join(REPO, "bin", "sample_autoregressive.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def abs_oracle():
    """The fp32 oracle on the weights of ref_abs_model.npz (hidden 64, 2 heads, 2 layers, absolute, 64 positions)."""
    gm = golden("ref_abs_model.npz")
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="absolute")
    om = ref_model.OracleBertForDiffusion(ocfg, [True] * 6)
    om.load_state_dict({k[4:]: torch.from_numpy(gm[k]) for k in gm.files if k.startswith("sd::")}, strict=True)
    return om


# ------------------------------------------------------------ the restatement against the reference class
def test_restated_forward_matches_the_reference_class():
    ga, om = golden("ref_autoregressive.npz"), abs_oracle()
    x = torch.from_numpy(ga["fwd_x"])
    mask = ar_reference.prefix_mask(ga["fwd_key_lens"].tolist(), x.shape[1])
    got = ar_reference.ar_forward(om, x, mask, torch.from_numpy(ga["fwd_seq_lengths"]))
    err = np.abs(got.numpy().astype(np.float64) - ga["fwd_out"]).max()
    print("restated forward vs reference class", err)
    assert err < GOLDEN_TOL


def test_restated_rollout_matches_the_reference_class():
    ga, om = golden("ref_autoregressive.npz"), abs_oracle()
    seed, lens, ns = torch.from_numpy(ga["seed"]), torch.from_numpy(ga["seq_lengths"]), int(ga["num_seed"])
    assert float(np.abs(ga["seed"][:, ns:]).max()) > 2.5   # the positions behind the seeds are not zeros
    items = ar_reference.ar_sample(om, seed, lens, ns)
    assert [tuple(i.shape) for i in items] == [(int(n), 6) for n in lens]
    full = ar_reference.ar_sample(om, seed, lens, ns, return_full=True)
    valid = ga["valid"]
    err = np.abs(full.numpy().astype(np.float64) - ga["rollout"])[valid].max()
    print("restated rollout vs reference class", err)
    assert err < GOLDEN_TOL
    assert torch.equal(full[:, :ns], seed[:, :ns])
    assert torch.equal(full[:, int(lens.max()):], seed[:, int(lens.max()):])


def test_rows_behind_the_step_influence_nothing():
    """Step i read over the rows 0 .. i only gives the rollout of the full-L forward (fp64: to rounding) -- the triangle
    the device loop runs."""
    ga = golden("ref_autoregressive.npz")
    om64 = ar_reference.as_double(abs_oracle(), 65)
    seed, lens, ns = torch.from_numpy(ga["seed"]).double(), torch.from_numpy(ga["seq_lengths"]), int(ga["num_seed"])
    full = ar_reference.ar_sample(om64, seed, lens, ns, return_full=True)
    tri = seed.clone()
    for i in range(ns, int(lens.max())):
        mask = torch.ones(seed.shape[0], i + 1, dtype=torch.float64)
        mask[:, i] = 0.0
        tri[:, i] = ar_reference.ar_forward(om64, tri[:, : i + 1], mask, lens)[:, i]
    err = (tri - full).abs().max().item()
    print("triangle vs square rollout, fp64", err)
    assert err < 1e-13


# ------------------------------------------------------------ the Python class
def _model(pos="relative_key", maxpos=32):
    cfg = modelling.BertConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1,
                               max_position_embeddings=maxpos, position_embedding_type=pos)
    return modelling.BertForAutoregressiveBase(cfg, [True] * 6)


def test_class_surface():
    m = _model()
    assert isinstance(m, modelling.BertForDiffusionBase)
    assert modelling.BertForAutoregressive is modelling.BertForAutoregressiveBase
    assert modelling.BertForAutoregressiveBase.from_dir.__func__ is modelling.BertForDiffusionBase.from_dir.__func__
    assert m.time_table(33).shape == (33, 64)


def test_argument_checks_come_before_the_device():
    m = _model()
    x = torch.zeros(2, 8, 6)
    lens = torch.tensor([8, 5])
    holed = ar_reference.prefix_mask([8, 5], 8)
    holed[0, 3] = 0.0
    with pytest.raises(NotImplementedError, match="prefix"):
        m.forward(x, holed, lens)
    with pytest.raises(NotImplementedError, match="prefix"):   # a sequence without a single key
        m.forward(x, ar_reference.prefix_mask([8, 0], 8), lens)
    with pytest.raises(NotImplementedError, match="position_ids"):
        m.forward(x, ar_reference.prefix_mask([8, 5], 8), lens, position_ids=torch.arange(8)[None])
    with pytest.raises(ValueError, match=r"\[0, 33\)"):
        m.forward(x, ar_reference.prefix_mask([8, 5], 8), torch.tensor([8, 33]))
    with pytest.raises(ValueError, match="sequence lengths"):
        m.forward(x, ar_reference.prefix_mask([8, 5], 8), torch.tensor([8]))
    with pytest.raises(ValueError, match="num_seed"):
        m.sample(x, lens, num_seed=0)
    with pytest.raises(ValueError, match="exceeds"):
        m.sample(x, torch.tensor([9, 5]), num_seed=2)
    with pytest.raises(ValueError, match=r"\[0, 33\)"):
        m.sample(x, torch.tensor([-1, 5]), num_seed=2)
    bad = x.clone()
    bad[1, 1, 2] = 3.2
    with pytest.raises(AssertionError):
        m.sample(bad, lens, num_seed=2)
    bad[1, 1, 2] = 0.0
    bad[1, 2, 2] = 3.2      # behind the seeds anything goes; the call then stops at the missing device
    for call in (lambda: m.sample(bad, lens, num_seed=2), lambda: m.forward(x, ar_reference.prefix_mask([8, 5], 8), lens)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ------------------------------------------------------------ the command line
def test_parser_takes_the_reference_scripts_arguments():
    """Option strings, types and defaults of the reference's build_parser, plus the required --seed_pdbs."""
    p = _cli().build_parser()
    by_dest = {a.dest: a for a in p._actions}
    want = {"model": ((), None, str), "outdir": (("-o", "--outdir"), ".", None), "num": (("--num",), 10, int),
            "num_angles": (("--num_angles",), 4, int), "lengths": (("-l", "--lengths"), [50, 128], int),
            "device": (("-d", "--device"), "cuda:0", str)}
    for dest, (flags, default, typ) in want.items():
        a = by_dest[dest]
        assert tuple(a.option_strings) == flags and a.default == default and a.type == typ, dest
    assert by_dest["lengths"].nargs == 2
    assert by_dest["seed_pdbs"].required
    with pytest.raises(SystemExit):
        p.parse_args(["some_model"])
    ns = p.parse_args(["some_model", "--seed_pdbs", "pdbs", "-l", "60", "62", "--num", "3"])
    assert (ns.model, ns.seed_pdbs, ns.lengths, ns.num, ns.num_angles, ns.outdir) == ("some_model", "pdbs", [60, 62], 3, 4, ".")


def test_sample_initial_angles_draw_order_and_values(tmp_path):
    """The file list is sorted, the draw is default_rng(seed).integers and row i holds the first n_angles residues of the
    i-th drawn file; noise comes from torch.manual_seed(seed).  The featurizer is injected: the default one runs on the
    device (test_autoregressive_gpu.py runs it on 1CRN.pdb)."""
    cli = _cli()
    names = ["b.pdb", "a.pdb", "c.pdb", "d.pdb", "e.pdb"]
    for n in names:
        (tmp_path / n).write_text("")
    rng = np.random.default_rng(3)
    table = {n: pd.DataFrame(rng.uniform(-3, 3, (7, 6)).astype(np.float32), columns=structures.EXHAUSTIVE_ANGLES) for n in names}
    seen = []

    def featurizer(fname):
        seen.append(os.path.basename(str(fname)))
        return table[seen[-1]]

    got = cli.sample_initial_angles(6, 4, eps=0.0, seed=1234, pdb_dir=str(tmp_path), featurizer=featurizer)
    order = [sorted(names)[i] for i in np.random.default_rng(1234).integers(0, 5, 6)]
    assert seen == order and len(set(order)) > 1
    assert got.shape == (6, 4, 6) and got.dtype == torch.float32
    for i, n in enumerate(order):
        assert np.array_equal(got[i].numpy(), ((table[n].values[:4] + np.pi) % (2 * np.pi) - np.pi).astype(np.float32))
    noisy = cli.sample_initial_angles(6, 4, eps=1e-2, seed=1234, pdb_dir=str(tmp_path), featurizer=featurizer)
    torch.manual_seed(1234)
    noise = torch.randn((6, 4, 6)) * 1e-2
    assert torch.allclose(noisy, got + noise, atol=1e-6) and not torch.equal(noisy, got)
    with pytest.raises(AssertionError, match="no files"):
        cli.sample_initial_angles(1, 4, pdb_dir=str(tmp_path / "missing"))
    assert os.path.isfile(os.path.join(GOLDEN, "1CRN.pdb"))


# ------------------------------------------------------------ the C entries
def test_entries_are_declared_and_reject_a_null_model(lib):
    """Both entries are in the header and the binding, and without a model they return -1 with "null" in fd_last_error()
    and leave the output alone -- all that can be asked without a device (no model can be created); the other argument
    checks need a model and are in tests/test_autoregressive_gpu.py."""
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    for name in ("fd_ar_forward", "fd_ar_sample"):
        assert re.search(r"\bint %s\(fd_model\* m," % name, header)
        assert name in _binding.exported_symbols() and hasattr(lib, name)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    x, out = np.zeros((2, 8, 6), np.float32), np.full((2, 8, 6), -7, np.float32)
    lens = np.array([8, 5], np.int32)
    assert lib.fd_ar_forward(None, P(x), P(lens), P(lens), 2, 8, P(out)) == -1 and b"null" in lib.fd_last_error()
    assert lib.fd_ar_sample(None, P(x), P(lens), 2, 8, 2, P(out)) == -1 and b"null" in lib.fd_last_error()
    assert (out == -7).all()
