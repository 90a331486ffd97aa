#!/usr/bin/env python3
"""MLM pretrainer step (pretrain_mlm.py:74-88,:144-166) on one MI355X: forward + CrossEntropyLoss over the
V = 64001 vocabulary + backward, bf16 tier, synthetic token ids with 15 % of the positions labelled.
    python tools/bench_mlm.py [--encoders 12] [--heads 12] [--batch 64] [--seq 512] [--steps 5] [--labelled-only {0,1}] [--labels {device,host}]
Prints one JSON line (secondary figure; the headline metric stays bench.py's).  --pairs N: N pairs of timed windows in this process,
the head on every row (--labelled-only 0) and on the labelled rows (1) alternating, one JSON line per window -- an A/B comparison
on one model, one warm-up and one set of inputs."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoders", type=int, default=12)
    ap.add_argument("--heads", type=int, default=12, help="12 -> Dh = 64 (flash path); the reference's default 8 -> Dh = 96 (zero-padded to the 128-wide kernels)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=64001)
    ap.add_argument("--labelled-only", type=int, choices=(0, 1), default=None,
                    help="1: the vocabulary head runs on the labelled rows alone; 0: on every row; default: the module's (MEANT_MLM_LABELLED_ONLY)")
    ap.add_argument("--labels", choices=("device", "host"), default="device", help="where the step finds its labels (host: no read-back of the row count)")
    ap.add_argument("--pairs", type=int, default=0, help="N > 0: alternate --labelled-only 0 and 1 windows N times in this process")
    args = ap.parse_args()
    import meant_amd as M
    from transformers import RobertaConfig, RobertaForMaskedLM
    dev = torch.device("cuda")
    cfg = RobertaConfig(vocab_size=args.vocab, hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=3072,
                        max_position_embeddings=args.seq + 2, pad_token_id=1, type_vocab_size=1, layer_norm_eps=1e-5)
    rob = RobertaForMaskedLM._from_config(cfg)
    model = M.meant_language_pretrainer(args.encoders, 768, rob.roberta.embeddings, rob.lm_head, text_dim=768, num_heads=args.heads).to(dev)
    model.compute_dtype = torch.bfloat16
    model.train()
    rs = np.random.RandomState(0)
    B, S, V = args.batch, args.seq, args.vocab
    ids = torch.from_numpy(rs.randint(2, V, (B, S))).to(dev)
    mask = torch.ones(B, S, device=dev)
    labels = torch.full((B, S), -100, dtype=torch.int64)
    pick = torch.from_numpy(rs.rand(B, S) < 0.15)
    labels[pick] = torch.from_numpy(rs.randint(2, V, int(pick.sum())))
    if args.labels == "device":
        labels = labels.to(dev)
    if args.labelled_only is not None:
        model.labelled_only = bool(args.labelled_only)

    # gradients go where meant_amd.train.TrainStep puts them: flat fp32 buckets, written by the backward kernels directly
    from meant_amd.parallel import GradReducer
    red = GradReducer(model.parameters(), direct_grads=True)

    def step():
        red.prepare()
        loss = model.loss(ids, mask, labels)
        loss.backward()
        red.wait()
        return loss

    T = B * S
    flops = 3 * (args.encoders * (16 * 768 * 768 * T + 4 * S * 768 * T) + 2 * 768 * 768 * T + 2 * 768 * V * T)

    def window(labelled_only):
        """warm-up (both routes have their own shapes) + one timed window; the algorithmic FLOP count is the all-rows step's either way"""
        model.labelled_only = labelled_only
        for _ in range(2):
            loss = step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        assert torch.isfinite(loss).item()
        print(json.dumps({"what": "MLM pretrainer fwd + CE(V) + bwd, bf16", "encoders": args.encoders, "heads": args.heads, "batch": B, "seq": S,
                          "vocab": V, "labelled_only": int(labelled_only), "labels": args.labels, "head_rows": model.last_head_rows,
                          "ms_per_step": round(dt * 1e3, 2), "tokens_per_s": round(T / dt, 1),
                          "tflops_algorithmic": round(flops / dt / 1e12, 1), "loss": round(loss.item(), 4)}), flush=True)

    if args.pairs > 0:
        for _ in range(args.pairs):
            window(False)
            window(True)
    else:
        window(model.labelled_only)


if __name__ == "__main__":
    main()
