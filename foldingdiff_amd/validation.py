"""
Evaluating a fixed checkpoint: the numbers the reference's ``validation_step`` / ``validation_epoch_end`` log
(foldingdiff/modelling.py:720-760), and the loss-against-timestep curve.

``validation_loss`` takes the noising from the host dataset (``NoisedAnglesDataset.__getitem__``: the reference's random
stream -- one ``torch.randint`` and one ``torch.randn_like`` per item from the global generator) and runs forward + loss as
one device call per batch (``BertForDiffusionBase.loss_terms``).  ``loss_by_timestep`` fixes the timestep of a whole pass
and noises on the device too (``fd_denoise_loss``).  Both honour the model's loss settings (``loss_key``,
``circle_lambda``, ``use_pairwise_dist_loss``): with the pairwise-distance term on there is one more value,
``pairwise_dist_loss``, as in the reference's ``validation_step``.  Forward only: no gradients, no optimizer.
"""
from typing import Dict, Optional, Sequence

import numpy as np
import torch


def _collate(items, keys):
    return {k: torch.stack([torch.as_tensor(it[k]) for it in items]) for k in keys}


def _unmasked(attn_mask: torch.Tensor) -> int:
    return int((attn_mask != 0).sum())


PAIRWISE_NAME = "pairwise_dist_loss"   # the pseudo feature name of validation_step (modelling.py:737-741)
_BATCH_KEYS = ("corrupted", "t", "known_noise", "attn_mask")
_PAIRWISE_KEYS = ("angles", "lengths", "sqrt_alphas_cumprod_t", "sqrt_one_minus_alphas_cumprod_t")


def _pairwise_on(model) -> bool:
    from . import losses
    return losses.pairwise_is_on(getattr(model, "use_pairwise_dist_loss", 0.0))


def _n_pairs(lengths: torch.Tensor) -> int:
    n = torch.as_tensor(lengths).reshape(-1).long()
    return int((n * (n - 1) // 2).sum())


@torch.no_grad()
def validation_loss(model, noised_dset, batch_size: int = 512) -> Dict[str, object]:
    """One pass over ``noised_dset`` (a ``NoisedAnglesDataset`` over real data) in index order, ``batch_size`` items per
    batch (the last one may be smaller), ``noised_dset[i]`` noised on the host.  Returns

    * ``"val_loss"``: the mean over batches of each batch's mean over features -- what ``validation_epoch_end`` logs;
    * ``"val_loss_<feature>"``: per feature, the mean over ALL unmasked positions of the pass (batches pooled by their
      position counts; with one batch this is ``validation_step``'s ``val_loss_<feature>``);
    * ``"per_batch"``: one ``{"n_items", "n_positions", "loss_terms": [F floats], "val_loss"}`` per batch.

    With the model's pairwise-distance term on, the batches also carry ``angles``, ``lengths`` and the two schedule
    coefficients, every batch has ``F + 1`` loss terms (``val_loss`` is the mean over all of them) and ``"n_pairs"``, and
    ``"val_loss_pairwise_dist_loss"`` is the mean over ALL CA pairs of the pass: batches pooled by their pair counts, not
    their position counts (a batch without pairs has a NaN term and no weight; NaN when the pass has no pairs)."""
    if batch_size < 1:
        raise ValueError(f"batch_size={batch_size}")
    names = list(noised_dset.feature_names[noised_dset.dset_key])
    pairwise = _pairwise_on(model)
    if hasattr(model, "prepare"):
        model.prepare(noised_dset.alpha_beta_terms["betas"])
    per_batch = []
    pooled, positions = np.zeros(len(names), np.float64), 0
    pooled_pairs, pairs = 0.0, 0
    for start in range(0, len(noised_dset), batch_size):
        items = [noised_dset[i] for i in range(start, min(start + batch_size, len(noised_dset)))]
        batch = _collate(items, _BATCH_KEYS + _PAIRWISE_KEYS if pairwise else _BATCH_KEYS)
        terms = np.asarray(model.loss_terms(batch), dtype=np.float64).reshape(-1)
        assert terms.shape == (len(names) + pairwise,), f"{terms.shape[0]} loss terms for {len(names)} features"
        n_pos = _unmasked(batch["attn_mask"])
        pooled += terms[:len(names)] * n_pos
        positions += n_pos
        per_batch.append({"n_items": len(items), "n_positions": n_pos, "loss_terms": [float(v) for v in terms],
                          "val_loss": float(terms.mean())})
        if pairwise:
            n_pairs = _n_pairs(batch["lengths"])
            per_batch[-1]["n_pairs"] = n_pairs
            if n_pairs:
                pooled_pairs += terms[-1] * n_pairs
                pairs += n_pairs
    if not per_batch:
        raise ValueError("empty dataset")
    out = {"val_loss": float(np.mean([b["val_loss"] for b in per_batch])), "per_batch": per_batch}
    for name, v in zip(names, pooled / positions):
        out[f"val_loss_{name}"] = float(v)
    if pairwise:
        out[f"val_loss_{PAIRWISE_NAME}"] = pooled_pairs / pairs if pairs else float("nan")
    return out


@torch.no_grad()
def loss_by_timestep(model, dset, timesteps: Sequence[int], batch_size: int = 512, seed: Optional[int] = 6489) -> np.ndarray:
    """The loss-against-timestep curve: float64 [len(timesteps), F] (one more column, the pairwise-distance term over
    all CA pairs, when the model has it on), row i the per-feature mean over all unmasked positions
    of ``dset`` with EVERY item noised to ``timesteps[i]``.  ``dset`` is a ``NoisedAnglesDataset``; the clean items come
    from the dataset it wraps and the noise from ``dset.sample_noise`` under a generator seeded with ``seed`` once per
    timestep (the same draw at every timestep, so the curve varies with t alone; None: the global generator's current
    state).  The noising x_t = keep x_0 + spread eps runs on the device (``fd_denoise_loss``)."""
    key = dset.dset_key
    terms_t = dset.alpha_beta_terms
    model.prepare(terms_t["betas"])
    clean = [dset.dset.__getitem__(i) for i in range(len(dset.dset))]
    x0 = torch.stack([it[key] for it in clean]).float()
    mask = torch.stack([it["attn_mask"] for it in clean])
    from . import losses
    F = x0.shape[2]
    pairwise = _pairwise_on(model)
    kind, lam = getattr(model, "loss_key", "smooth_l1"), float(getattr(model, "circle_lambda", 0.0))
    circle = kind == "smooth_l1" and lam > 0
    plain = kind == "smooth_l1" and not circle and not pairwise
    out = np.zeros((len(timesteps), F + pairwise), np.float64)
    for row, t in enumerate(timesteps):
        if not 0 <= int(t) < dset.timesteps:
            raise ValueError(f"timestep {t} outside [0, {dset.timesteps})")
        if seed is not None:
            torch.manual_seed(seed)
        keep = terms_t["sqrt_alphas_cumprod"][int(t)].float().reshape(1)
        spread = terms_t["sqrt_one_minus_alphas_cumprod"][int(t)].float().reshape(1)
        positions, pairs = 0, 0
        for start in range(0, x0.shape[0], batch_size):
            xb, mb = x0[start:start + batch_size], mask[start:start + batch_size]
            B = xb.shape[0]
            eps = torch.stack([dset.sample_noise(xb[i]) for i in range(B)])
            tb = torch.full((B,), int(t), dtype=torch.long)
            if plain:
                sums = model.denoise_loss_sums(xb, eps, tb, mb, keep=keep.expand(B), spread=spread.expand(B))
                out[row] += sums.sum(axis=0)
            else:
                coef = losses.pairwise_coef(model.use_pairwise_dist_loss, tb) if pairwise else None
                got = model.denoise_loss_ex(xb, eps, tb, mb, keep=keep.expand(B), spread=spread.expand(B), kind=kind,
                                            return_turns=circle, pairwise=pairwise, coef=coef)
                out[row, :F] += got["sums"].sum(axis=0)
                if circle:
                    out[row, :F] += lam * got["turns"].sum(axis=0)
                if pairwise:
                    out[row, F] += got["pair_sums"].sum()
                    pairs += int(got["pairs"].sum())
            positions += _unmasked(mb)
        out[row, :F] /= positions
        if pairwise:
            out[row, F] = out[row, F] / pairs if pairs else np.nan
    return out
