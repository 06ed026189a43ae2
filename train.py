#!/usr/bin/env python3
"""Command-line trainer with the reference's `train` arguments (reference train.py:183-189, `make train`):

    python train.py --config diffusion_handwriting_generation/configs/best.yml [--data batches.pt] [--out runs/exp]

Runs the reference's TrainingLoop (train.py:84-134) with every update on the MI355X (dhg_amd.train_model: one replayed
hipGraph per update; under torch.distributed.run one process per GPU with an RCCL all-reduce of the gradients).  The config
is the reference's yml (training_args: steps, batch_size, warmup_steps, clip_grad, dropout, att_layers_num, channels,
log_freq, save_freq; dataset_args: max_seq_len, max_text_len; optimizer.params: betas, weight_decay).  `--data`: a torch file
{"strokes" [N,L,3], "text" [N,Lt] int64, "style" [N,14,1280]} of preprocessed samples (the reference's IAMDataset items,
dataset.py:143-157; read with weights_only=True); without it, synthetic batches of the configured shape (smoke / benchmark
runs — the IAM corpus and its preprocessing are outside this package).  Writes checkpoint_<n>.pth in save_checkpoint's form
({"meta": None, "state_dict": ...}, reference checkpoint.py:244) and model_final.pth as the bare state_dict (train.py:131),
both with the reference's 323 keys; cadence and numbering follow the reference ((count + 1) % freq, see fit()).
`--resident` uploads the --data set once (with its optional "writer" key, int [N]) and draws and gathers every batch on the GPU inside
the replayed graph; a sample's style then comes from a random other line of the same writer (dataset.py:110-115).
`--cond-drop P` hides the prompt and the writer of a sample with probability P (conditioning dropout, drawn on the GPU inside the graph),
which is what gives a checkpoint the unconditional branch that `infer.py --guidance` extrapolates from.
`--ema D` keeps the exponential moving average of the weights inside the optimizer's pass and writes ema_<n>.pth / ema_final.pth;
`--save-state` keeps train_state.pth (weights, Adam's moments and counter, the EMA) and `--resume PATH` continues from one;
`--val batches.pt [--eval-freq N]` logs the held-out loss at fixed noise levels (and, with --ema, that of the averaged weights).
--precision bf16 selects the mixed-precision GEMMs (fp32 master weights and optimizer state); batch_size is per rank."""
import argparse

import dhg_amd


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True)
    ap.add_argument("--data")
    ap.add_argument("--resident", action="store_true", help="keep the --data set on the GPU and draw every batch there (style from another line of the same writer)")
    ap.add_argument("--out", default="runs/exp")
    ap.add_argument("--steps", type=int, help="override training_args.steps")
    ap.add_argument("--init", help="state_dict to start from (.pth)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"], help="GEMM operand precision (fp32 = the reference's)")
    ap.add_argument("--cond-drop", type=float, default=0.0, metavar="P",
                    help="conditioning dropout: with probability P a sample trains without its prompt and writer (for infer.py --guidance; 0.1 is customary)")
    ap.add_argument("--ema", type=float, metavar="D", help="keep an exponential moving average of the weights with decay D in (0, 1) (0.9999 is customary); "
                    "writes ema_<n>.pth and ema_final.pth, the weights to sample from")
    ap.add_argument("--save-state", action="store_true", help="keep train_state.pth in --out: weights, Adam's moments and counter, the EMA (for --resume)")
    ap.add_argument("--resume", metavar="PATH", help="continue the run a train_state.pth was saved from (implies --save-state)")
    ap.add_argument("--val", metavar="PATH", help="validation set (the form of --data): log its loss at fixed noise levels as `Eval <n> | ...` lines")
    ap.add_argument("--eval-freq", type=int, metavar="N", help="evaluate --val every N updates (default: training_args.save_freq)")
    a = ap.parse_args(argv)
    if not 0.0 <= a.cond_drop <= 1.0:
        ap.error("--cond-drop must lie in [0, 1]")
    if a.ema is not None and not 0.0 < a.ema < 1.0:
        ap.error("--ema must lie in (0, 1)")
    if a.eval_freq is not None and (a.eval_freq < 1 or not a.val):
        ap.error("--eval-freq must be a positive number of updates and needs --val")
    dhg_amd.train_model.fit(a.config, a.data, a.out, steps=a.steps, init=a.init, seed=a.seed, precision=a.precision, resident=a.resident,
                            cond_drop=a.cond_drop, ema=a.ema, save_state=a.save_state or a.resume is not None, resume=a.resume, val_path=a.val,
                            eval_freq=a.eval_freq)


if __name__ == "__main__":
    main()
