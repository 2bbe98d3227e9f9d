"""Host side of the denoising loss (no GPU): the torch restatements against the reference's golden terms, the new C-ABI
entries' declarations and argument checks, and the batch logic of validation.validation_loss on a stub model."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from foldingdiff_amd import _binding, losses, validation

NEW_ENTRIES = ("fd_forward_t", "fd_loss_terms", "fd_denoise_loss")


@pytest.fixture(scope="module")
def gl():
    return golden("ref_loss.npz")


def test_host_restatements_equal_the_reference_terms_bit_for_bit(gl):
    """The same torch operations on the same host class as the fixture: every per-position term of the golden batch and
    of the synthetic seam / threshold set has the reference's bits, and so have the six means of _get_loss_terms when the
    reference's predicted noise is put in."""
    ang = [bool(a) for a in gl["ft_is_angular"]]
    pred, target = torch.from_numpy(gl["pred"]), torch.from_numpy(gl["known_noise"])
    got = losses.host_terms(pred, target, ang).numpy()
    assert got.dtype == np.float32 and np.array_equal(got, gl["terms"])
    sp, st = torch.from_numpy(gl["syn_pred"]), torch.from_numpy(gl["syn_target"])
    for p, t, a, l in zip(sp, st, gl["syn_terms_ang"], gl["syn_terms_lin"]):
        assert losses.radian_smooth_l1_loss(p.reshape(1), t.reshape(1), beta=losses.ANGULAR_BETA).item() == a
        assert losses.smooth_l1_loss(p.reshape(1), t.reshape(1)).item() == l
    assert losses.ANGULAR_BETA == float(gl["beta_ang"]) and losses.NONANGULAR_BETA == float(gl["beta_lin"])
    # the synthetic set does what it is for: both branches, and differences beyond the seam that the wrap brings back
    d = (st - sp).double()
    assert (gl["syn_terms_ang"] < 0.5 * losses.ANGULAR_BETA).any() and (gl["syn_terms_ang"] > 2.98).any()   # (at most pi - beta / 2)
    assert ((d.abs() > np.pi) & (torch.from_numpy(gl["syn_terms_ang"]).double() < 0.2)).any()
    # _get_loss_terms: per feature the mean over the unmasked positions (masked selection, then torch.mean)
    idx = torch.where(torch.from_numpy(gl["attn_mask"]))
    for f, a in enumerate(ang):
        p, t = pred[idx[0], idx[1], f], target[idx[0], idx[1], f]
        v = losses.radian_smooth_l1_loss(p, t, beta=losses.ANGULAR_BETA) if a else losses.smooth_l1_loss(p, t)
        assert v.item() == gl["ref_loss_terms"][f]


def test_doctest_value_and_unbuilt_options():
    v = losses.radian_smooth_l1_loss(torch.tensor(-17.0466), torch.tensor(-1.3888), beta=0.1)
    assert f"{v.item():.4f}" == "3.0414"
    with pytest.raises(NotImplementedError, match="circle_penalty"):
        losses.radian_smooth_l1_loss(torch.zeros(2), torch.zeros(2), circle_penalty=0.1)
    assert losses.radian_smooth_l1_loss(torch.zeros(2), torch.zeros(2), circle_penalty=0.0).item() == 0.0


def test_new_entries_are_declared_and_exported(lib):
    src = open(os.path.join(REPO, "include", "fdmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fd_[a-z_0-9]+)\s*\(", src))
    for name in NEW_ENTRIES:
        assert name in declared, f"{name} is not declared in include/fdmi.h"
        assert name in _binding.exported_symbols(), f"{name} is not bound"
        assert hasattr(lib, name), f"{name} is not exported by libfdmi.so"
    assert lib.fd_abi_version() == _binding.ABI_VERSION   # (additive entries: the version itself did not move)


def test_fd_loss_terms_rejects_bad_arguments_before_touching_a_device(lib):
    """Every bad call returns -1 with its word in fd_last_error() and leaves both outputs at the sentinel, on a machine
    without a GPU too.  No valid call is made.  B = 2, L = 6, F = 3."""
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    pred, target = np.zeros((2, 6, 3), np.float32), np.ones((2, 6, 3), np.float32)
    lens, flags = np.array([6, 2], np.int32), np.array([1, 0, 1], np.uint8)
    checked = 0

    def call(pred=pred, target=target, lens=lens, B=2, L=6, F=3, flags=flags, ba=0.3, bl=1.0, sums="default", terms="default"):
        sums = np.full((2, 3), -7.0) if isinstance(sums, str) else sums
        terms = np.full((2, 6, 3), -7, np.float32) if isinstance(terms, str) else terms
        rc = lib.fd_loss_terms(0, P(pred), P(target), P(lens), B, L, F, P(flags), C.c_float(ba), C.c_float(bl), P(sums), P(terms))
        return [sums, terms], rc

    for kw, word in [(dict(pred=None), b"null"), (dict(target=None), b"null"), (dict(lens=None), b"null"),
                     (dict(flags=None), b"null"), (dict(sums=None), b"null"), (dict(B=0), b"B=0"), (dict(L=0), b"L=0"),
                     (dict(lens=np.array([6, 0], np.int32)), b"lens"), (dict(lens=np.array([7, 2], np.int32)), b"outside [1, 6]"),
                     (dict(F=0), b"F=0"), (dict(F=33), b"F=33"), (dict(ba=0.0), b"beta"), (dict(ba=-1.0), b"beta"),
                     (dict(bl=0.0), b"beta"), (dict(ba=float("nan")), b"beta")]:
        outs, rc = call(**kw)
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (kw.keys(), word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)
        checked += 1
    assert checked == 15
    # the model entries check their model first: a null model is an error code, never a fault
    sums = np.full((2, 3), -7.0)
    t = np.zeros(2, np.int32)
    assert lib.fd_forward_t(None, P(pred), P(t), P(lens), 2, 6, P(target.copy())) == -1 and b"null" in lib.fd_last_error()
    assert lib.fd_denoise_loss(None, P(pred), P(target), P(t), None, None, P(lens), 2, 6, C.c_float(0.3), C.c_float(1.0),
                               P(sums), None, None) == -1 and b"null" in lib.fd_last_error()
    assert (sums == -7).all()


def test_loss_terms_wrapper_checks_shapes_before_the_library():
    z = np.zeros((2, 6, 3), np.float32)
    with pytest.raises(ValueError, match="angular flags"):
        losses.loss_terms(z, z, [6, 2], [True, False])
    with pytest.raises(ValueError, match="same"):
        losses.loss_terms(z, z[:, :5], [6, 2], [True, False, True])
    with pytest.raises(ValueError, match="prefix mask"):
        losses.loss_terms(z, z, np.array([[1, 1, 0, 1, 0, 0], [1, 0, 0, 0, 0, 0]]), [True, False, True])
    assert losses.lengths_of(torch.tensor([[1., 1, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0]]), 6).tolist() == [3, 1]


class _ToyDset:
    """Seven items of lengths 1..7 at pad 8, two features; item i's noising is recognisable from its values."""
    dset_key = "angles"
    feature_names = {"angles": ["phi", "d0"]}
    alpha_beta_terms = {"betas": torch.linspace(1e-4, 0.02, 10)}

    def __len__(self):
        return 7

    def __getitem__(self, i):
        if not 0 <= i < 7:
            raise IndexError(i)
        mask = torch.zeros(8)
        mask[: i + 1] = 1.0
        return {"corrupted": torch.full((8, 2), float(i)), "known_noise": torch.full((8, 2), float(-i)), "t": torch.tensor([i]),
                "attn_mask": mask, "angles": torch.zeros(8, 2)}


class _StubModel:
    """loss_terms is canned: feature 0 = the mean item index of the batch, feature 1 = 10 x the number of items."""
    def __init__(self):
        self.batches, self.prepared = [], 0

    def prepare(self, betas):
        self.prepared += 1

    def loss_terms(self, batch):
        self.batches.append({k: v.clone() for k, v in batch.items()})
        idx = batch["corrupted"][:, 0, 0]
        assert torch.equal(batch["known_noise"][:, 0, 0], -idx) and torch.equal(batch["t"].reshape(-1).float(), idx)
        return torch.tensor([idx.double().mean().item(), 10.0 * len(idx)], dtype=torch.float64)


def test_validation_loss_splits_batches_in_order_and_takes_both_means():
    m = _StubModel()
    out = validation.validation_loss(m, _ToyDset(), batch_size=3)
    assert m.prepared == 1
    assert [b["corrupted"][:, 0, 0].tolist() for b in m.batches] == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0], [6.0]]
    assert [tuple(b["attn_mask"].shape) for b in m.batches] == [(3, 8), (3, 8), (1, 8)]
    assert set(m.batches[0]) == {"corrupted", "t", "known_noise", "attn_mask"}
    terms = [[1.0, 30.0], [4.0, 30.0], [6.0, 10.0]]
    npos = [1 + 2 + 3, 4 + 5 + 6, 7]
    assert [b["loss_terms"] for b in out["per_batch"]] == terms
    assert [b["n_positions"] for b in out["per_batch"]] == npos and [b["n_items"] for b in out["per_batch"]] == [3, 3, 1]
    # val_loss: mean over batches of the mean over features (validation_epoch_end over validation_step's avg_loss)
    assert out["val_loss"] == pytest.approx(np.mean([np.mean(t) for t in terms]), rel=1e-15)
    # per feature: pooled over every unmasked position of the pass
    for f, name in enumerate(["phi", "d0"]):
        want = sum(t[f] * n for t, n in zip(terms, npos)) / sum(npos)
        assert out[f"val_loss_{name}"] == pytest.approx(want, rel=1e-15)
    assert out["val_loss_phi"] != pytest.approx(np.mean([t[0] for t in terms]))   # (the two means differ on ragged batches)
    one = validation.validation_loss(_StubModel(), _ToyDset(), batch_size=512)
    assert len(one["per_batch"]) == 1 and one["val_loss_phi"] == 3.0 and one["val_loss"] == (3.0 + 70.0) / 2
    with pytest.raises(ValueError):
        validation.validation_loss(_StubModel(), _ToyDset(), batch_size=0)
