#!/usr/bin/env python3
"""
Generate tests/golden/ref_autoregressive.npz by running THE REFERENCE's ``BertForAutoregressiveBase`` itself
(needs the reference checkout, see make_golden.py; the output is committed because the GPU machine has none):

    python tests/golden/make_golden_autoregressive.py

The model is the reference class on the weights already in ref_abs_model.npz (hidden 64, 2 heads, 2 layers, absolute
positions, 64 positions), built through ``make_golden.import_reference()`` with the same ``init_weights`` stub as
make_golden.py.  Recorded:
  fwd_x, fwd_key_lens, fwd_seq_lengths, fwd_out   one ``forward`` with prefix keys
  seed, seq_lengths, num_seed, rollout            one ``sample``: lengths [48, 31, 40, 7], 3 seeds, seed values uniform
                                                  in +-3 at EVERY position (row i enters step i with them); ``rollout``
                                                  is the full [B, L, F] state, rebuilt from the returned list over ``seed``
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import make_golden  # noqa: E402


def main():
    _, _, modelling, _, _ = make_golden.import_reference()
    from transformers import BertConfig

    import ar_reference
    from oracle import ref_model

    gm = np.load(os.path.join(HERE, "ref_abs_model.npz"))
    sd = {k[4:]: torch.from_numpy(gm[k]) for k in gm.files if k.startswith("sd::")}
    modelling.BertForDiffusionBase.init_weights = lambda self: None  # broken under transformers 5.x
    cfg = BertConfig(max_position_embeddings=64, num_attention_heads=2, hidden_size=64, intermediate_size=128,
                     num_hidden_layers=2, position_embedding_type="absolute", hidden_dropout_prob=0.1,
                     attention_probs_dropout_prob=0.1, use_cache=False, attn_implementation="eager")
    ref = modelling.BertForAutoregressiveBase(cfg, ft_is_angular=[True] * 6, time_encoding="gaussian_fourier", decoder="mlp")
    ref.load_state_dict(sd, strict=True)
    ref.eval()

    g = torch.Generator().manual_seed(8642)
    B, L = 4, 48
    fwd_x = (torch.rand(B, L, 6, generator=g) * 2 - 1) * 3.0
    fwd_key_lens = [48, 1, 33, 8]
    fwd_seq_lengths = torch.tensor([48, 64, 0, 17])
    with torch.no_grad():
        fwd_out = ref(fwd_x, attention_mask=ar_reference.prefix_mask(fwd_key_lens, L), seq_lengths=fwd_seq_lengths)

    seq_lengths = torch.tensor([48, 31, 40, 7])
    num_seed = 3
    seed = (torch.rand(B, L, 6, generator=g) * 2 - 1) * 3.0
    items = ref.sample(seed.clone(), seq_lengths, num_seed=num_seed, pbar=False)
    # every sequence runs to max(seq_lengths) inside the loop and the returned list is trimmed: the fixture holds what
    # the reference returns, laid over the seed, and `valid` marks the positions it returned
    rollout = seed.clone()
    for b, it in enumerate(items):
        rollout[b, : it.shape[0]] = it
    valid = ar_reference.prefix_mask(seq_lengths.tolist(), L).bool().numpy()

    # the restatement must reproduce the reference class (the gate of make_golden.py / test_oracle_golden.py)
    ocfg = ref_model.OracleConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                                  max_position_embeddings=64, position_embedding_type="absolute")
    om = ref_model.OracleBertForDiffusion(ocfg, [True] * 6)
    om.load_state_dict(sd, strict=True)
    d_fwd = (ar_reference.ar_forward(om, fwd_x, ar_reference.prefix_mask(fwd_key_lens, L), fwd_seq_lengths) - fwd_out).abs().max().item()
    full = ar_reference.ar_sample(om, seed, seq_lengths, num_seed, return_full=True)
    d_roll = (full - rollout).abs().numpy()[valid].max()
    print(f"[autoregressive] restatement vs reference class: forward {d_fwd:.3e}, rollout {d_roll:.3e}")
    assert d_fwd < 5e-6 and d_roll < 5e-6
    out = os.path.join(HERE, "ref_autoregressive.npz")
    np.savez_compressed(out, fwd_x=fwd_x.numpy(), fwd_key_lens=np.array(fwd_key_lens), fwd_seq_lengths=fwd_seq_lengths.numpy(),
                        fwd_out=fwd_out.numpy(), seed=seed.numpy(), seq_lengths=seq_lengths.numpy(), num_seed=num_seed,
                        rollout=rollout.numpy(), valid=valid)
    print(f"{out}: {os.path.getsize(out) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
