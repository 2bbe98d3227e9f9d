#!/usr/bin/env python3
"""
Golden fixture for the denoising loss, produced by THE REFERENCE:
  * ``NoisedAnglesDataset.__getitem__(idx, use_t_val=...)`` (foldingdiff/datasets.py:801-886) on the small synthetic
    angle dataset of make_golden_noising.py, here with four angular and two non-angular features and one timestep per
    item (0, 17, 999, 17, 503), fixed torch seed;
  * ``BertForDiffusion._get_loss_terms`` (foldingdiff/modelling.py:553-604), called unbound on the reference
    ``BertForDiffusionBase`` (absolute positions) whose weights are in ref_abs_model.npz, with ``loss_func`` = the
    "smooth_l1" pair, ``circle_lambda = 0`` and ``use_pairwise_dist_loss = 0`` set on it; the predicted noise of the
    same forward;
  * ``losses.radian_smooth_l1_loss(beta = pi / 10)`` and ``F.smooth_l1_loss`` on one-element tensors: the per-position
    terms of that batch, and of a synthetic set whose differences sit within 1e-3 of +-pi and of +-beta on both sides.
Writes tests/golden/ref_loss.npz.  Needs the reference checkout (FD_REFERENCE, as make_golden.py finds it):

    python tests/golden/make_golden_loss.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
mg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mg)

PAD, F, T, SEED = 48, 6, 1000, 4242
LENGTHS = [48, 31, 40, 7, 19]
TIMESTEPS = [0, 17, 999, 17, 503]
ANGULAR = [True] * 4 + [False] * 2


class ToyAngles(torch.utils.data.Dataset):
    """Stand-in for CathCanonicalAnglesDataset: items are dicts with zero-padded [pad, F] features."""
    feature_names = {"angles": ["phi", "psi", "omega", "tau", "d0", "d1"]}
    feature_is_angular = {"angles": list(ANGULAR)}
    pad = PAD

    def __init__(self, angles):
        self.angles = angles
        self.filenames = [f"toy_{i}.pdb" for i in range(len(LENGTHS))]

    def __len__(self):
        return len(LENGTHS)

    def __getitem__(self, index, ignore_zero_center=False):
        l = LENGTHS[index]
        mask = torch.zeros(PAD)
        mask[:l] = 1.0
        return {"angles": self.angles[index].clone(), "attn_mask": mask, "position_ids": torch.arange(PAD),
                "lengths": torch.tensor(l, dtype=torch.int64)}


def synthetic_differences():
    """(pred, target) float32 pairs whose difference target - pred sits near the places the term changes branch: within 1e-3
    of +-pi (the wrap seam) and of +-beta for beta = pi / 10 and 1 (the quadratic / linear switch), on both sides, plus
    multiples of 2 pi away and a spread of ordinary values.  No exact ties: every offset is an odd multiple of 1e-5."""
    g = torch.Generator().manual_seed(31)
    offs = torch.tensor([1e-5, 3e-5, 11e-5, 37e-5, 99e-5], dtype=torch.float64)
    centres = torch.tensor([np.pi, -np.pi, np.pi / 10, -np.pi / 10, 1.0, -1.0, 0.0, 3 * np.pi, -3 * np.pi,
                            2 * np.pi + np.pi / 10, -2 * np.pi - np.pi / 10], dtype=torch.float64)
    d = torch.cat([(centres[:, None] + offs[None, :]).reshape(-1), (centres[:, None] - offs[None, :]).reshape(-1),
                   torch.randn(90, generator=g, dtype=torch.float64) * 2.5])
    pred = torch.randn(d.numel(), generator=g, dtype=torch.float64) * 1.5
    pred, target = pred.float(), (pred + d).float()
    return pred, target


def main():
    mg.import_reference()
    sys.path.insert(0, mg.REF)
    from foldingdiff import datasets, losses, modelling, utils
    from torch.nn import functional as Fn
    from torch.utils.data.dataloader import default_collate
    from transformers import BertConfig

    g = torch.Generator().manual_seed(99)
    angles = torch.zeros(len(LENGTHS), PAD, F)
    for i, l in enumerate(LENGTHS):
        angles[i, :l] = torch.randn(l, F, generator=g) * 1.3
        angles[i, :l, :4] = utils.modulo_with_wrapped_range(angles[i, :l, :4], -np.pi, np.pi)
    dset = datasets.NoisedAnglesDataset(ToyAngles(angles), dset_key="angles", timesteps=T, beta_schedule="cosine")

    gm = np.load(os.path.join(HERE, "ref_abs_model.npz"))
    modelling.BertForDiffusionBase.init_weights = lambda self: None  # broken under transformers 5.x
    cfg = BertConfig(max_position_embeddings=64, num_attention_heads=2, hidden_size=64, intermediate_size=128,
                     num_hidden_layers=2, position_embedding_type="absolute", hidden_dropout_prob=0.1,
                     attention_probs_dropout_prob=0.1, use_cache=False, attn_implementation="eager")
    model = modelling.BertForDiffusionBase(cfg, ft_is_angular=list(ANGULAR), time_encoding="gaussian_fourier", decoder="mlp")
    model.load_state_dict({k[4:]: torch.from_numpy(gm[k]) for k in gm.files if k.startswith("sd::")}, strict=True)
    model.eval()
    # what BertForDiffusion.__init__ sets for loss="smooth_l1", circle_reg=0, use_pairwise_dist_loss=0 (modelling.py:510-543)
    model.loss_func = [modelling.BertForDiffusion.angular_loss_fn_dict["smooth_l1"] if a
                       else modelling.BertForDiffusion.nonangular_loss_fn_dict["smooth_l1"] for a in model.ft_is_angular]
    model.circle_lambda = 0.0
    model.use_pairwise_dist_loss = 0.0

    out = {"angles": angles.numpy(), "lengths": np.array(LENGTHS), "timesteps": np.array(TIMESTEPS), "seed": SEED, "T": T,
           "pad": PAD, "ft_is_angular": np.array(ANGULAR), "beta_ang": np.float64(torch.pi / 10), "beta_lin": np.float64(1.0)}
    torch.manual_seed(SEED)
    items = [dset.__getitem__(i, use_t_val=t) for i, t in enumerate(TIMESTEPS)]
    batch = default_collate(items)
    for k in ("corrupted", "known_noise", "t", "attn_mask", "sqrt_alphas_cumprod_t", "sqrt_one_minus_alphas_cumprod_t"):
        out[k] = batch[k].numpy().copy()
    assert out["sqrt_alphas_cumprod_t"].dtype == np.float32
    with torch.no_grad():
        out["ref_loss_terms"] = modelling.BertForDiffusion._get_loss_terms(model, batch).numpy()
        pred = model.forward(batch["corrupted"], batch["t"], attention_mask=batch["attn_mask"], position_ids=batch["position_ids"])
    out["pred"] = pred.numpy().copy()

    ang_fn, lin_fn = model.loss_func[0], Fn.smooth_l1_loss

    def one(fn, p, t):  # the mean over a one-element tensor is the term itself
        return float(fn(p.reshape(1), t.reshape(1)))

    terms = torch.zeros_like(pred)
    for b in range(pred.shape[0]):
        for l in range(PAD):
            for f in range(F):
                terms[b, l, f] = one(ang_fn if ANGULAR[f] else lin_fn, pred[b, l, f], batch["known_noise"][b, l, f])
    out["terms"] = terms.numpy()
    sp, st = synthetic_differences()
    out["syn_pred"], out["syn_target"] = sp.numpy(), st.numpy()
    out["syn_terms_ang"] = np.array([one(ang_fn, p, t) for p, t in zip(sp, st)], np.float32)
    out["syn_terms_lin"] = np.array([one(lin_fn, p, t) for p, t in zip(sp, st)], np.float32)
    # float(): a one-element float32 mean widened exactly; stored back as float32
    assert np.array_equal(out["terms"].astype(np.float64).astype(np.float32), out["terms"])
    path = os.path.join(HERE, "ref_loss.npz")
    np.savez_compressed(path, **out)
    print("ref_loss.npz:", os.path.getsize(path) / 1024, "KiB; t =", out["t"].reshape(-1).tolist(), "terms =", out["ref_loss_terms"])
    print("doctest:", losses.radian_smooth_l1_loss(torch.tensor(-17.0466), torch.tensor(-1.3888), beta=0.1))


if __name__ == "__main__":
    main()
