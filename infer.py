#!/usr/bin/env python3
"""Command-line sampler with the reference's `infer` arguments (reference inference.py:19-27, `make infer`):

    python infer.py "Follow the White Rabbit" style.npy --experiment-path data/best_exp --output result

`source` is a handwriting image of the writer (as in the reference: cropped, resized to 96 rows, MobileNetV2 StyleExtractor;
`--style-weights` = a local copy of torchvision's mobilenet_v2 checkpoint) or a file with the writer-style features
([14,1280], .npy or .pt).

Many lines of one writer in one batched sampler call (each line at its own stroke length), written to <output>_<i>.png:

    python infer.py --prompts-file lines.txt style.npy --experiment-path data/best_exp --output page"""
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
    a = ap.parse_args(argv)
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
        out = dhg_amd.infer_file_batch(prompts, source, a.config_path, a.checkpoint_path, a.experiment_path, a.output,
                                       a.diffusion_mode, precision=a.precision, seed=a.seed, style_weights=a.style_weights, renderer=a.renderer)
        for i, s in enumerate(out):
            print(f"{s.shape[0]} stroke points -> ./{a.output}_{i}.png")
        return
    if a.prompt is None or a.source is None:
        ap.error("the following arguments are required: prompt, source")
    strokes = dhg_amd.infer_file(a.prompt, a.source, a.config_path, a.checkpoint_path, a.experiment_path, a.output,
                                 a.diffusion_mode, precision=a.precision, seed=a.seed, style_weights=a.style_weights, renderer=a.renderer)
    print(f"{strokes.shape[0]} stroke points -> ./{a.output}.png")


if __name__ == "__main__":
    main()
