"""
Evaluating a fixed checkpoint: the numbers the reference's ``validation_step`` / ``validation_epoch_end`` log
(foldingdiff/modelling.py:720-760), and the loss-against-timestep curve.

``validation_loss`` takes the noising from the host dataset (``NoisedAnglesDataset.__getitem__``: the reference's random
stream -- one ``torch.randint`` and one ``torch.randn_like`` per item from the global generator) and runs forward + loss as
one device call per batch (``BertForDiffusionBase.loss_terms``).  ``loss_by_timestep`` fixes the timestep of a whole pass
and noises on the device too (``fd_denoise_loss``).  Forward only: no gradients, no optimizer.
"""
from typing import Dict, Optional, Sequence

import numpy as np
import torch


def _collate(items, keys):
    return {k: torch.stack([torch.as_tensor(it[k]) for it in items]) for k in keys}


def _unmasked(attn_mask: torch.Tensor) -> int:
    return int((attn_mask != 0).sum())


@torch.no_grad()
def validation_loss(model, noised_dset, batch_size: int = 512) -> Dict[str, object]:
    """One pass over ``noised_dset`` (a ``NoisedAnglesDataset`` over real data) in index order, ``batch_size`` items per
    batch (the last one may be smaller), ``noised_dset[i]`` noised on the host.  Returns

    * ``"val_loss"``: the mean over batches of each batch's mean over features -- what ``validation_epoch_end`` logs;
    * ``"val_loss_<feature>"``: per feature, the mean over ALL unmasked positions of the pass (batches pooled by their
      position counts; with one batch this is ``validation_step``'s ``val_loss_<feature>``);
    * ``"per_batch"``: one ``{"n_items", "n_positions", "loss_terms": [F floats], "val_loss"}`` per batch."""
    if batch_size < 1:
        raise ValueError(f"batch_size={batch_size}")
    names = list(noised_dset.feature_names[noised_dset.dset_key])
    if hasattr(model, "prepare"):
        model.prepare(noised_dset.alpha_beta_terms["betas"])
    per_batch = []
    pooled, positions = np.zeros(len(names), np.float64), 0
    for start in range(0, len(noised_dset), batch_size):
        items = [noised_dset[i] for i in range(start, min(start + batch_size, len(noised_dset)))]
        batch = _collate(items, ("corrupted", "t", "known_noise", "attn_mask"))
        terms = np.asarray(model.loss_terms(batch), dtype=np.float64).reshape(-1)
        assert terms.shape == (len(names),), f"{terms.shape[0]} loss terms for {len(names)} features"
        n_pos = _unmasked(batch["attn_mask"])
        pooled += terms * n_pos
        positions += n_pos
        per_batch.append({"n_items": len(items), "n_positions": n_pos, "loss_terms": [float(v) for v in terms],
                          "val_loss": float(terms.mean())})
    if not per_batch:
        raise ValueError("empty dataset")
    out = {"val_loss": float(np.mean([b["val_loss"] for b in per_batch])), "per_batch": per_batch}
    for name, v in zip(names, pooled / positions):
        out[f"val_loss_{name}"] = float(v)
    return out


@torch.no_grad()
def loss_by_timestep(model, dset, timesteps: Sequence[int], batch_size: int = 512, seed: Optional[int] = 6489) -> np.ndarray:
    """The loss-against-timestep curve: float64 [len(timesteps), F], row i the per-feature mean over all unmasked positions
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
    out = np.zeros((len(timesteps), x0.shape[2]), np.float64)
    for row, t in enumerate(timesteps):
        if not 0 <= int(t) < dset.timesteps:
            raise ValueError(f"timestep {t} outside [0, {dset.timesteps})")
        if seed is not None:
            torch.manual_seed(seed)
        keep = terms_t["sqrt_alphas_cumprod"][int(t)].float().reshape(1)
        spread = terms_t["sqrt_one_minus_alphas_cumprod"][int(t)].float().reshape(1)
        positions = 0
        for start in range(0, x0.shape[0], batch_size):
            xb, mb = x0[start:start + batch_size], mask[start:start + batch_size]
            B = xb.shape[0]
            eps = torch.stack([dset.sample_noise(xb[i]) for i in range(B)])
            sums = model.denoise_loss_sums(xb, eps, torch.full((B,), int(t), dtype=torch.long), mb,
                                           keep=keep.expand(B), spread=spread.expand(B))
            out[row] += sums.sum(axis=0)
            positions += _unmasked(mb)
        out[row] /= positions
    return out
