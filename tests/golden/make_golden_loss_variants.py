#!/usr/bin/env python3
"""
Golden fixture for the rest of the denoising loss, produced by THE REFERENCE: the "l1" loss, the circle penalty and the
pairwise-distance term of ``BertForDiffusion._get_loss_terms`` (foldingdiff/modelling.py:553-679).

Two toy batches of the six canonical angles (phi, psi, omega, tau, CA:C:1N, C:1N:1CA; all angular), noised by
``NoisedAnglesDataset.__getitem__(idx, use_t_val=...)`` under a fixed torch seed:

  s1   PAD = 48,  lengths 48, 1, 2, 3, 31, timesteps 0, 17, 60, 17, 100; predicted noise of the reference
       ``BertForDiffusionBase`` (absolute positions) whose weights are in ref_abs_model.npz, all features angular
  s2   PAD = 128, lengths 128, 65, timesteps 40, 5; that model has 64 positions, so the predicted noise is the fp32
       oracle's (oracle/ref_model.py, relative_key, hidden 192, 6 heads, seed 23) and ``_get_loss_terms`` is called
       on a stand-in whose ``forward`` returns that recorded prediction -- every line of the loss is still the reference's

The timesteps stay <= 100: ``keep`` falls toward 0 at high t and the denoised angles then amplify any difference in the
forward without bound, so a comparison there says nothing about the loss code.

Per batch: the batch itself (angles, corrupted, known_noise, t, attn_mask, lengths, both coefficient vectors), ``pred``,
``_get_loss_terms`` (called unbound) for the settings "l1" / "smooth_l1" with circle_lambda = 0.3 /
use_pairwise_dist_loss = (0.05, 0.5, 1000) / everything off, the per-position ``radian_l1_loss`` terms and
trunc(|pred| / pi) from one-element calls, and -- fed the recorded ``pred`` -- the denoised angles, both
``nerf_build_batch`` CA traces, the coefficient, ``pairwise_dist_loss`` per sequence (one sequence per call), for the
batch, and with a 0-dim tensor weight (the scalar form of the coefficient, which the reference's own caller cannot
reach: it asks a python float for ``.ndim``).
Plus a synthetic set for the l1 term and the turn count at the places they change: differences within 1e-3 of +-pi,
inputs within 1e-3 of 0 and of multiples of +-2 pi (the remainder's seam), |pred| within 1e-3 of multiples of pi.

The script asserts what the tests lean on: every unmasked |pred| is at least 1e-3 away from a multiple k >= 1 of pi
(no turn count can flip under a forward error of 1e-5; with these weights |pred| stays below pi, so every count of the
two batches is 0 and the counts are exercised by the synthetic set), and every sequence with pairs has an RMS
pair-distance difference that a relative gate can resolve.  The RMS values are printed.  With the lengths and timesteps
above the reference gives 0.25, 0.04, 0.13, 2.1 A (s1) and 4.0, 1.4 A (s2): a sequence of two or three residues at
t <= 60 moves its CA atoms by a tenth of an Angstrom at most, whatever the seed.  The floor asserted is RMS_FLOOR = 0.01 A:
the distances are stored as float32 (half an ulp is 2.4e-7 A at 4 .. 8 A), so at 0.01 A a difference still carries
four digits and its square three -- far more than the gates of the tests need.
Writes tests/golden/ref_loss_variants.npz.  Needs the reference checkout (FD_REFERENCE, as make_golden.py finds it):

    python tests/golden/make_golden_loss_variants.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
mg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mg)

F, T, SEED = 6, 1000, 4243
NAMES = ["phi", "psi", "omega", "tau", "CA:C:1N", "C:1N:1CA"]
SETS = {"s1": (48, [48, 1, 2, 3, 31], [0, 17, 60, 17, 100], 99),
        "s2": (128, [128, 65], [40, 5], 100)}
CIRCLE, PDIST, SCALAR_COEF, RMS_FLOOR = 0.3, (0.05, 0.5, 1000), 0.25, 0.01
ORACLE_S2 = dict(hidden=192, heads=6, seed=23)


class ToyAngles(torch.utils.data.Dataset):
    """Stand-in for CathCanonicalAnglesDataset: items are dicts with zero-padded [pad, F] features."""
    feature_names = {"angles": list(NAMES)}
    feature_is_angular = {"angles": [True] * F}

    def __init__(self, angles, lengths):
        self.angles, self.lengths, self.pad = angles, lengths, angles.shape[1]
        self.filenames = [f"toy_{i}.pdb" for i in range(len(lengths))]

    def __len__(self):
        return len(self.lengths)

    def __getitem__(self, index, ignore_zero_center=False):
        l = self.lengths[index]
        mask = torch.zeros(self.pad)
        mask[:l] = 1.0
        return {"angles": self.angles[index].clone(), "attn_mask": mask, "position_ids": torch.arange(self.pad),
                "lengths": torch.tensor(l, dtype=torch.int64)}


def synthetic_l1():
    """(pred, target) float32 pairs at the places the l1 term and the turn count change.  No exact ties: every offset is
    an odd multiple of 1e-5."""
    g = torch.Generator().manual_seed(37)
    offs = torch.tensor([1e-5, 3e-5, 11e-5, 37e-5, 99e-5], dtype=torch.float64)
    both = lambda c: torch.cat([(c[:, None] + offs[None, :]).reshape(-1), (c[:, None] - offs[None, :]).reshape(-1)])  # noqa: E731
    pi = np.pi
    # differences target - pred near +-pi (and a turn further), from ordinary preds
    d = both(torch.tensor([pi, -pi, 3 * pi, -3 * pi, 0.0], dtype=torch.float64))
    p1 = torch.randn(d.numel(), generator=g, dtype=torch.float64) * 1.5
    t1 = p1 + d
    # inputs at the remainder's seam: pred and target near 0, +-2 pi, +-4 pi, paired with ordinary partners and each other
    seam = both(torch.tensor([0.0, 2 * pi, -2 * pi, 4 * pi, -4 * pi], dtype=torch.float64))
    p2 = torch.cat([seam, torch.randn(seam.numel(), generator=g, dtype=torch.float64) * 2.0, seam])
    t2 = torch.cat([torch.randn(seam.numel(), generator=g, dtype=torch.float64) * 2.0, seam, seam.flip(0)])
    # |pred| near the multiples of pi (the turn count steps there)
    p3 = both(torch.tensor([pi, -pi, 2 * pi, -2 * pi, 3 * pi, -3 * pi, 5 * pi, 0.0], dtype=torch.float64))
    t3 = torch.randn(p3.numel(), generator=g, dtype=torch.float64) * 1.5
    # a spread of ordinary values
    p4 = torch.randn(90, generator=g, dtype=torch.float64) * 4.0
    t4 = torch.randn(90, generator=g, dtype=torch.float64) * 4.0
    return torch.cat([p1, p2, p3, p4]).float(), torch.cat([t1, t2, t3, t4]).float()


def main():
    mg.import_reference()
    sys.path.insert(0, mg.REF)
    sys.path.insert(0, mg.REPO)
    from foldingdiff import datasets, losses, modelling, nerf, utils
    from torch.nn import functional as Fn
    from torch.utils.data.dataloader import default_collate
    from transformers import BertConfig
    from oracle import ref_model

    gm = np.load(os.path.join(HERE, "ref_abs_model.npz"))
    modelling.BertForDiffusionBase.init_weights = lambda self: None  # broken under transformers 5.x
    cfg = BertConfig(max_position_embeddings=64, num_attention_heads=2, hidden_size=64, intermediate_size=128,
                     num_hidden_layers=2, position_embedding_type="absolute", hidden_dropout_prob=0.1,
                     attention_probs_dropout_prob=0.1, use_cache=False, attn_implementation="eager")
    ref = modelling.BertForDiffusionBase(cfg, ft_is_angular=[True] * F, ft_names=list(NAMES),
                                         time_encoding="gaussian_fourier", decoder="mlp")
    ref.load_state_dict({k[4:]: torch.from_numpy(gm[k]) for k in gm.files if k.startswith("sd::")}, strict=True)
    ref.eval()
    ocfg = ref_model.OracleConfig(hidden_size=ORACLE_S2["hidden"], num_attention_heads=ORACLE_S2["heads"],
                                  intermediate_size=2 * ORACLE_S2["hidden"], num_hidden_layers=2,
                                  max_position_embeddings=128, position_embedding_type="relative_key")
    o32 = ref_model.synthetic_model(ocfg, (True,) * F, "gaussian_fourier", "mlp", seed=ORACLE_S2["seed"])

    loss_lists = {k: [modelling.BertForDiffusion.angular_loss_fn_dict[k]] * F for k in ("l1", "smooth_l1")}

    def one(fn, p, t):  # the mean over a one-element tensor is the term itself
        return float(fn(p.reshape(1), t.reshape(1)))

    def turns_of(p):
        return torch.div(torch.abs(p), torch.pi, rounding_mode="trunc")

    out = {"T": T, "seed": SEED, "names": np.array(NAMES), "circle_lambda": np.float64(CIRCLE),
           "pdist": np.array(PDIST, np.float64), "scalar_coef": np.float64(SCALAR_COEF),
           "oracle_s2": np.array([ORACLE_S2["hidden"], ORACLE_S2["heads"], ORACLE_S2["seed"]])}
    for tag, (pad, lengths, timesteps, aseed) in SETS.items():
        g = torch.Generator().manual_seed(aseed)
        angles = torch.zeros(len(lengths), pad, F)
        for i, l in enumerate(lengths):
            angles[i, :l] = utils.modulo_with_wrapped_range(torch.randn(l, F, generator=g) * 1.3, -np.pi, np.pi)
        dset = datasets.NoisedAnglesDataset(ToyAngles(angles, lengths), dset_key="angles", timesteps=T, beta_schedule="cosine")
        torch.manual_seed(SEED)
        batch = default_collate([dset.__getitem__(i, use_t_val=t) for i, t in enumerate(timesteps)])
        with torch.no_grad():
            if tag == "s1":
                pred = ref.forward(batch["corrupted"], batch["t"], attention_mask=batch["attn_mask"], position_ids=batch["position_ids"])
            else:
                pred = o32(batch["corrupted"], batch["t"], attention_mask=batch["attn_mask"]).float()
        pred = pred.detach().clone()
        # _get_loss_terms unbound, on an object whose forward returns the recorded prediction (s1: the reference model's
        # own forward gives the same tensor; checked below)
        shim = types.SimpleNamespace(forward=lambda *a, **k: pred, ft_names=list(NAMES))

        def terms_for(loss, circle, pdist, me=shim):
            me.loss_func, me.circle_lambda, me.use_pairwise_dist_loss = loss_lists[loss], circle, pdist
            with torch.no_grad():
                return modelling.BertForDiffusion._get_loss_terms(me, batch).numpy().copy()

        o = {"angles": angles.numpy(), "lengths": np.array(lengths), "timesteps": np.array(timesteps), "pred": pred.numpy()}
        for k in ("corrupted", "known_noise", "t", "attn_mask", "sqrt_alphas_cumprod_t", "sqrt_one_minus_alphas_cumprod_t"):
            o[k] = batch[k].numpy().copy()
        assert o["sqrt_alphas_cumprod_t"].dtype == np.float32 and np.array_equal(batch["lengths"].numpy(), lengths)
        o["ref_l1"] = terms_for("l1", 0.0, 0.0)
        o["ref_circle"] = terms_for("smooth_l1", CIRCLE, 0.0)
        o["ref_pdist"] = terms_for("smooth_l1", 0.0, PDIST)
        o["ref_plain"] = terms_for("smooth_l1", 0.0, 0.0)
        assert o["ref_pdist"].shape == (F + 1,) and np.array_equal(o["ref_pdist"][:F], o["ref_plain"])
        if tag == "s1":   # the stand-in changes nothing: the reference model itself gives the same numbers
            assert np.array_equal(terms_for("smooth_l1", CIRCLE, PDIST, me=ref), np.append(o["ref_circle"], o["ref_pdist"][F]))
        unmasked = batch["attn_mask"].bool()
        q = torch.abs(pred[unmasked].double()) / np.pi   # the count steps at |pred| = k pi, k >= 1 (not at 0)
        away = torch.abs(q - torch.clamp(torch.round(q), min=1.0)).min().item() * np.pi
        print(f"{tag}: unmasked |pred| is at least {away:.3e} away from a multiple k >= 1 of pi; turns up to {turns_of(pred[unmasked]).max().item():.0f}")
        assert away >= 1e-3

        l1 = torch.zeros_like(pred)
        for b in range(pred.shape[0]):
            for l in range(pad):
                for f in range(F):
                    l1[b, l, f] = one(losses.radian_l1_loss, pred[b, l, f], batch["known_noise"][b, l, f])
        o["terms_l1"] = l1.numpy()
        assert np.array_equal(o["terms_l1"].astype(np.float64).astype(np.float32), o["terms_l1"])
        o["turns"] = turns_of(pred).numpy().astype(np.int32)

        # the pairwise-distance term piece by piece, the statements of modelling.py:621-676 on the recorded pred
        bs = pred.shape[0]
        den = batch["corrupted"] - batch["sqrt_one_minus_alphas_cumprod_t"].view(bs, 1, 1) * pred
        den /= batch["sqrt_alphas_cumprod_t"].view(bs, 1, 1)
        cols = lambda a: dict(phi=a[:, :, 0], psi=a[:, :, 1], omega=a[:, :, 2], bond_angle_n_ca_c=a[:, :, 3],  # noqa: E731
                              bond_angle_ca_c_n=a[:, :, 4], bond_angle_c_n_ca=a[:, :, 5])
        with torch.no_grad():
            xyz_clean, xyz_den = nerf.nerf_build_batch(**cols(batch["angles"])), nerf.nerf_build_batch(**cols(den))
        assert xyz_clean.dtype == torch.float64 and xyz_clean.shape == (bs, 3 * pad, 3)
        ca_idx = torch.arange(start=1, end=xyz_den.shape[1], step=3)
        ca_clean, ca_den = xyz_clean[:, ca_idx, :].detach(), xyz_den[:, ca_idx, :].detach()
        mn, mx, mt = PDIST
        coef = mn + (mx - mn) * ((mt - batch["t"]) / mt)
        assert coef.dtype == torch.float32 and coef.shape == (bs, 1)
        lens_t = batch["lengths"]
        per_seq = [float(losses.pairwise_dist_loss(ca_den[b:b + 1], ca_clean[b:b + 1], lengths=lens_t[b:b + 1], weights=coef[b:b + 1]))
                   for b in range(bs)]
        o["denoised"], o["ca_clean"], o["ca_denoised"], o["coef"] = den.numpy(), ca_clean.numpy(), ca_den.numpy(), coef.numpy()
        o["pd_per_seq"] = np.array(per_seq, np.float32)
        assert np.array_equal(o["pd_per_seq"].astype(np.float64), np.array(per_seq), equal_nan=True)
        o["pd_batch"] = losses.pairwise_dist_loss(ca_den, ca_clean, lengths=lens_t, weights=coef).numpy()
        assert o["pd_batch"] == o["ref_pdist"][F]
        o["pd_scalar"] = losses.pairwise_dist_loss(ca_den, ca_clean, lengths=lens_t, weights=torch.tensor(SCALAR_COEF)).numpy()
        o["pd_scalar_per_seq"] = np.array([float(losses.pairwise_dist_loss(ca_den[b:b + 1], ca_clean[b:b + 1], lengths=lens_t[b:b + 1],
                                                                           weights=torch.tensor(SCALAR_COEF))) for b in range(bs)], np.float32)
        rms = []
        for b, l in enumerate(lengths):
            if l < 2:
                assert np.isnan(per_seq[b])
                continue
            dd = Fn.pdist(ca_den[b, :l]) - Fn.pdist(ca_clean[b, :l])
            rms.append(float(torch.sqrt(torch.mean(dd * dd))))
        print(f"{tag}: RMS pair-distance difference per sequence with pairs (A):", [round(r, 3) for r in rms])
        assert min(rms) >= RMS_FLOOR, rms
        print(f"{tag}: l1 {o['ref_l1']}\n    circle {o['ref_circle']}\n    pdist {o['ref_pdist'][F]} per seq {per_seq} scalar {o['pd_scalar']}")
        out.update({f"{tag}::{k}": v for k, v in o.items()})

    sp, st = synthetic_l1()
    out["syn_pred"], out["syn_target"] = sp.numpy(), st.numpy()
    out["syn_terms_l1_ang"] = np.array([one(losses.radian_l1_loss, p, t) for p, t in zip(sp, st)], np.float32)
    out["syn_terms_l1_lin"] = np.array([one(Fn.l1_loss, p, t) for p, t in zip(sp, st)], np.float32)
    out["syn_turns"] = turns_of(sp).numpy().astype(np.int32)
    path = os.path.join(HERE, "ref_loss_variants.npz")
    np.savez_compressed(path, **out)
    print("ref_loss_variants.npz:", os.path.getsize(path) / 1024, "KiB;", len(sp), "synthetic pairs, turns", np.bincount(out["syn_turns"]))


if __name__ == "__main__":
    main()
