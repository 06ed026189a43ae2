#!/usr/bin/env python3
"""Command-line sampler with the reference's `infer` arguments (reference inference.py:19-27, `make infer`):

    python infer.py "Follow the White Rabbit" style.npy --experiment-path data/best_exp --output result

`source` is a handwriting image of the writer (as in the reference: cropped, resized to 96 rows, MobileNetV2 StyleExtractor;
`--style-weights` = a local copy of torchvision's mobilenet_v2 checkpoint) or a file with the writer-style features
([14,1280], .npy or .pt).

Many lines of one writer in one batched sampler call (each line at its own stroke length), written to <output>_<i>.png:

    python infer.py --prompts-file lines.txt style.npy --experiment-path data/best_exp --output page

The same lines in another writer's hand (restyling: the strokes an earlier run saved are noised `--strength` of the way up the
schedule and denoised under the new style, so the layout stays and the hand changes):

    python infer.py --prompts-file lines.txt style.npy --experiment-path data/best_exp --save-strokes lines.npy
    python infer.py --prompts-file lines.txt other.npy --experiment-path data/best_exp --restyle lines.npy --strength 0.5

Every line as the best of N samples under the model's own denoising objective, and that objective for saved lines (one
"length, score term, pen term, total" per prompt, lower fits better; no images):

    python infer.py --prompts-file lines.txt style.npy --experiment-path data/best_exp --candidates 8
    python infer.py --prompts-file lines.txt style.npy --experiment-path data/best_exp --score lines.npy

Where each character of saved lines sits, from the model's cross attention ("line i: 'c' rows a..b" per token; writes
<output>_align.npz with mean, token and lengths, and no images):

    python infer.py --prompts-file lines.txt style.npy --experiment-path data/best_exp --align lines.npy

Deterministic sampling at N of the schedule's levels (DDIM, eta = 0: N denoiser calls instead of 60, no noise after the start):

    python infer.py "Follow the White Rabbit" style.npy --experiment-path data/best_exp --steps 20
    python infer.py "Follow the White Rabbit" style.npy --experiment-path data/best_exp --steps 10 --order 2

Classifier-free guidance (a checkpoint trained with `train.py --cond-drop`; works with or without --steps, --prompts-file, --page-file):

    python infer.py "Follow the White Rabbit" style.npy --experiment-path data/best_exp --guidance 2.5

A whole text as pages (word-wrapped, every line at the same scale, composed on the GPU into <output>_p<k>.png):

    python infer.py --page-file letter.txt style.npy --experiment-path data/best_exp --output letter

The pages as curves too (<output>_p<k>.svg next to each PNG: for pen plotters, print at any size, drawing programs):

    python infer.py --page-file letter.txt style.npy --experiment-path data/best_exp --output letter --svg

Ground truth for the pages (<output>_p<k>.json next to each PNG: the box, stroke rows and text of every word; for training
recognition, word-spotting and layout models; --truth-level char: every character; --truth-labels: also <output>_p<k>_labels.npy,
the item every ink pixel belongs to):

    python infer.py --page-file letter.txt style.npy --experiment-path data/best_exp --output letter --truth"""
import argparse

import dhg_amd


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("prompt", nargs="?", help="the text to write (omitted with --prompts-file)")
    ap.add_argument("source", nargs="?")
    ap.add_argument("--prompts-file", help="one prompt per line (blank lines skipped), all sampled in one call")
    ap.add_argument("--config-path")
    ap.add_argument("--checkpoint-path")
    ap.add_argument("--experiment-path")
    ap.add_argument("--output", default="result")
    ap.add_argument("--diffusion-mode", default="new", choices=["new", "standard"])
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--style-weights", help="torchvision mobilenet_v2 state_dict (.pth) for the StyleExtractor")
    ap.add_argument("--renderer", default="matplotlib", choices=list(dhg_amd.inference.RENDERERS),
                    help="how the PNGs are drawn: the reference's matplotlib figure, or the 96-row grey line image rasterised on the GPU")
    ap.add_argument("--save-strokes", metavar="NPY", help="also write the sampled strokes, [B, max L, 3] padded with 0, to this .npy")
    ap.add_argument("--restyle", metavar="NPY", help="strokes of these prompts from an earlier run (--save-strokes): rewrite them in the hand of `source`")
    ap.add_argument("--strength", type=float, default=0.5, help="--restyle: share of the schedule the old strokes are noised up (0..1, default 0.5)")
    ap.add_argument("--candidates", type=int, default=1, metavar="N", help="sample every prompt N times and keep the candidate the model scores best")
    ap.add_argument("--score", metavar="NPY", help="strokes of these prompts from an earlier run (--save-strokes): print how well each line fits its "
                                                   "text and the hand of `source` under the model; writes no images")
    ap.add_argument("--align", metavar="NPY", help="strokes of these prompts from an earlier run (--save-strokes): print the stroke rows the model's "
                                                   "cross attention assigns to every character and write <output>_align.npz; writes no images")
    ap.add_argument("--steps", type=int, default=None, metavar="N", help="sample deterministically (DDIM, eta = 0) at N evenly spread levels of the "
                                                                         "schedule instead of the stochastic reverse process over all of them")
    ap.add_argument("--order", type=int, default=None, choices=(1, 2), help="with --steps: 1 = DDIM, 2 = the second-order multistep solver (DPM-Solver++ 2M) "
                                                                          "over the same levels, the same number of denoiser calls")
    ap.add_argument("--guidance", type=float, default=None, metavar="W", help="classifier-free guidance scale (1 = unguided, larger = closer to the prompt "
                                                                              "and the writer); needs a checkpoint trained with train.py --cond-drop")
    ap.add_argument("--page-file", metavar="TXT", help="a text to write as pages: wrapped to lines, every line sampled, all lines composed on the "
                                                       "GPU at one shared scale into <output>_p<k>.png (a blank line leaves a gap)")
    ap.add_argument("--svg", action="store_true", help="with --page-file: also write every page as curves to <output>_p<k>.svg")
    ap.add_argument("--truth", action="store_true", help="with --page-file: also write every page's word boxes, stroke rows and text to "
                                                         "<output>_p<k>.json")
    ap.add_argument("--truth-level", default=None, choices=("word", "char"), help="with --truth: boxes of words (default) or of characters")
    ap.add_argument("--truth-labels", action="store_true", help="with --truth: also the per-pixel map of item ids, <output>_p<k>_labels.npy")
    a = ap.parse_args(argv)
    if a.svg and not a.page_file:
        ap.error("--svg writes pages as curves: it needs --page-file")
    if a.truth and not a.page_file:
        ap.error("--truth writes the ground truth of pages: it needs --page-file")
    if (a.truth_level or a.truth_labels) and not a.truth:
        ap.error("--truth-level and --truth-labels say what --truth writes: pass --truth")
    if a.page_file and (a.score or a.align or a.restyle):
        ap.error("--page-file writes a text: it goes with neither --score, --align nor --restyle")
    if a.page_file and a.prompts_file:
        ap.error("--page-file and --prompts-file are two ways to give the text: pass one")
    if not 0.0 <= a.strength <= 1.0:
        ap.error("--strength must lie in [0, 1]")
    if a.candidates < 1:
        ap.error("--candidates must be at least 1")
    if a.score and (a.restyle or a.candidates > 1 or a.save_strokes):
        ap.error("--score only reads: it goes with neither --restyle, --candidates nor --save-strokes")
    if a.align and (a.score or a.restyle or a.candidates > 1 or a.save_strokes):
        ap.error("--align only reads: it goes with neither --score, --restyle, --candidates nor --save-strokes")
    if a.align and not a.prompts_file:
        ap.error("--align needs --prompts-file: the lines the strokes were sampled for")
    if a.restyle and a.candidates > 1:
        ap.error("--candidates belongs to sampling, not to --restyle")
    if a.steps is not None and a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.order is not None and a.steps is None:
        ap.error("--order chooses the solver of deterministic sampling: it needs --steps")
    if a.steps is not None and (a.score or a.align or a.restyle):
        ap.error("--steps belongs to sampling: it goes with neither --score, --align nor --restyle")

    def report(prompts, source):
        rows = dhg_amd.score_file(prompts, a.score, source, a.config_path, a.checkpoint_path, a.experiment_path, precision=a.precision,
                                  seed=a.seed, style_weights=a.style_weights)
        for i, (n, s_, p_, t_) in enumerate(rows):
            print(f"line {i}: length {n} score {s_:.6g} pen {p_:.6g} total {t_:.6g}")

    def report_align(prompts, source):
        import numpy as np
        al, ids, lens = dhg_amd.align_file(prompts, a.align, source, a.config_path, a.checkpoint_path, a.experiment_path, precision=a.precision,
                                           style_weights=a.style_weights)
        tok = dhg_amd.Tokenizer()
        for i, spans in enumerate(al.spans):
            for k, tid in enumerate(ids[i]):
                ch = tok.decode([tid])
                where = f"rows {spans[k][0]}..{spans[k][1]}" if spans[k] is not None else "no rows"
                print(f"line {i}: {ch!r} {where}")
        np.savez(f"{a.output}_align.npz", mean=np.asarray(al.mean), token=np.asarray(al.token), lengths=np.asarray(lens, np.int32))
        print(f"alignment of {len(lens)} lines -> ./{a.output}_align.npz")

    if a.guidance is not None and not 0.0 <= a.guidance <= dhg_amd.inference.MAX_GUIDANCE:
        ap.error(f"--guidance must lie in [0, {dhg_amd.inference.MAX_GUIDANCE:g}]")
    if a.guidance is not None and (a.score or a.align or a.restyle or a.candidates > 1):
        ap.error("--guidance belongs to plain sampling: it goes with neither --score, --align, --restyle nor --candidates")

    cand = dict(candidates=a.candidates) if a.candidates > 1 else {}   # (candidates = 1: today's calls, argument for argument)
    if a.steps is not None:
        cand["steps"] = a.steps
    if a.order is not None:
        cand["order"] = a.order
    if a.guidance is not None:
        cand["guidance"] = a.guidance

    def save(strokes_list):
        if a.save_strokes:
            import numpy as np
            np.save(a.save_strokes, dhg_amd.pad_strokes(strokes_list))
            print(f"strokes {len(strokes_list)} x [L,3] -> {a.save_strokes}")

    if a.page_file:
        if a.prompt is not None and a.source is not None:
            ap.error("with --page-file pass only the source")
        source = a.source if a.source is not None else a.prompt
        if source is None:
            ap.error("the source (handwriting image or style features) is required")
        with open(a.page_file, encoding="utf-8") as f:
            text = f.read()
        if not text.split():
            ap.error(f"{a.page_file} holds no word")
        out = dhg_amd.write_page_file(text, source, a.config_path, a.checkpoint_path, a.experiment_path, a.output, a.diffusion_mode,
                                      precision=a.precision, seed=a.seed, style_weights=a.style_weights, **cand, **(dict(svg=True) if a.svg else {}),
                                      **(dict(truth=True, truth_level=a.truth_level or "word", truth_labels=a.truth_labels) if a.truth else {}))
        save(out)
        print(f"{len(out)} lines -> ./{a.output}_p<k>.png" + (f" and ./{a.output}_p<k>.svg" if a.svg else "")
              + (f" and ./{a.output}_p<k>.json" if a.truth else ""))
        return
    if a.prompts_file:
        if a.prompt is not None and a.source is not None:
            ap.error("with --prompts-file pass only the source")
        source = a.source if a.source is not None else a.prompt
        if source is None:
            ap.error("the source (handwriting image or style features) is required")
        with open(a.prompts_file, encoding="utf-8") as f:
            prompts = [ln.rstrip("\r\n") for ln in f if ln.strip()]
        if not prompts:
            ap.error(f"{a.prompts_file} holds no prompt")
        if a.score:
            return report(prompts, source)
        if a.align:
            return report_align(prompts, source)
        if a.restyle:
            out = dhg_amd.restyle_file(prompts, a.restyle, source, a.config_path, a.checkpoint_path, a.experiment_path, a.output,
                                       a.diffusion_mode, strength=a.strength, precision=a.precision, seed=a.seed,
                                       style_weights=a.style_weights, renderer=a.renderer)
        else:
            out = dhg_amd.infer_file_batch(prompts, source, a.config_path, a.checkpoint_path, a.experiment_path, a.output,
                                           a.diffusion_mode, precision=a.precision, seed=a.seed, style_weights=a.style_weights, renderer=a.renderer,
                                           **cand)
        save(out)
        for i, s in enumerate(out):
            print(f"{s.shape[0]} stroke points -> ./{a.output}_{i}.png")
        return
    if a.prompt is None or a.source is None:
        ap.error("the following arguments are required: prompt, source")
    if a.score:
        return report([a.prompt], a.source)
    if a.restyle:
        (strokes,) = dhg_amd.restyle_file([a.prompt], a.restyle, a.source, a.config_path, a.checkpoint_path, a.experiment_path, a.output,
                                          a.diffusion_mode, strength=a.strength, precision=a.precision, seed=a.seed,
                                          style_weights=a.style_weights, renderer=a.renderer)
        save([strokes])
        print(f"{strokes.shape[0]} stroke points -> ./{a.output}_0.png")
        return
    strokes = dhg_amd.infer_file(a.prompt, a.source, a.config_path, a.checkpoint_path, a.experiment_path, a.output,
                                 a.diffusion_mode, precision=a.precision, seed=a.seed, style_weights=a.style_weights, renderer=a.renderer, **cand)
    save([strokes])
    print(f"{strokes.shape[0]} stroke points -> ./{a.output}.png")


if __name__ == "__main__":
    main()
