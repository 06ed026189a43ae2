#!/usr/bin/env python3
"""Reduce the printed figures of tests/test_gpu_blocks.py (pytest -s) to one line per RUN of the ragged and store-policy cases
(profiles/block_ratios_ragged.txt); the full print is one line per run, precision and tap - 6564 lines for these runs.

    python -m pytest tests/test_gpu_blocks.py -m gpu -s -q > blocks.log
    python tools/block_ratios.py blocks.log > profiles/block_ratios_ragged.txt

With `text` as second argument: the text-shape cases (text_*) and the PLANE lines of tests/test_gpu_text_plane.py instead
(profiles/block_ratios_text.txt):

    python -m pytest tests/test_gpu_blocks.py tests/test_gpu_text_plane.py -m gpu -s -q > text.log
    python tools/block_ratios.py text.log text > profiles/block_ratios_text.txt

bf16 run:  <case[+r<k>]> bf16 taps <n> row <smallest>..<largest device / model ratio> (<tap of the largest>) max <smallest>..<largest>
           (<tap>) exact <largest abs error of the float32-exact taps>
fp32 run:  <case[+r<k>]> fp32 taps <n> abs <largest abs error> (<tap>)       (set k of a case is another list of lengths per precision)
"""
import sys


def main():
    text = sys.argv[2:] == ["text"]
    runs = {}
    for line in open(sys.argv[1]):
        word = next((w for w in (("BLOCKS ", "PLANE ") if text else ("BLOCKS ",)) if w in line and line.lstrip(".sFEx").startswith(w)), None)
        if word is None:   # (pytest's progress marks run into the print)
            continue
        p = line[line.index(word):].split()
        case, prec, tap = p[1], p[2], p[3]
        if p[0] == "PLANE" and len(p) < 6:
            continue
        if (not (case.startswith("text_") or p[0] == "PLANE")) if text else ("+r" not in case and not case.startswith("pol")):
            continue
        r = runs.setdefault((case, prec), dict(n=0, row=[], max=[], abs=[]))
        r["n"] += 1
        if p[4] == "abs":
            r["abs"].append((float(p[5]), tap))
        else:
            r["row"].append((float(p[6]), tap))
            r["max"].append((float(p[9]), tap))
    if text:
        print("# tests/test_gpu_blocks.py (text-shape cases text_*) and tests/test_gpu_text_plane.py (P*) on the MI355X, one line per run:")
    else:
        print("# tests/test_gpu_blocks.py on the MI355X, ragged runs (<case>+r<k>) and store-policy cases (pol<word>_<case>), one line per run:")
    print("# reduced by tools/block_ratios.py from the printed BLOCKS lines (format in its docstring)")
    for (case, prec), r in runs.items():
        if prec == "fp32":
            print(f"{case} fp32 taps {r['n']} abs {max(r['abs'])[0]:.3e} ({max(r['abs'])[1]})")
        else:
            exact = f" exact {max(r['abs'])[0]:.3e}" if r["abs"] else ""
            print(f"{case} bf16 taps {r['n']} row {min(r['row'])[0]:.2f}..{max(r['row'])[0]:.2f} ({max(r['row'])[1]}) "
                  f"max {min(r['max'])[0]:.2f}..{max(r['max'])[0]:.2f} ({max(r['max'])[1]}){exact}")
    if text:   # what the next change of the text side is judged against: the largest fp32 error per tap, the bf16 runs above 1.5
        worst = {}
        for (case, prec), r in runs.items():
            if prec == "fp32":
                for v, tap in r["abs"]:
                    if v > worst.get(tap, (0.0, ""))[0]:
                        worst[tap] = (v, case)
        print("# largest fp32 absolute error per tap over all runs above:")
        for tap, (v, case) in sorted(worst.items()):
            print(f"fp32-worst {tap} {v:.3e} ({case})")
        print("# bf16 runs whose largest device / model ratio exceeds 1.5 (bound: 2):")
        for (case, prec), r in runs.items():
            if prec == "bf16":
                for kind in ("row", "max"):
                    if r[kind] and max(r[kind])[0] > 1.5:
                        print(f"above-1.5 {case} {kind} {max(r[kind])[0]:.2f} ({max(r[kind])[1]})")


if __name__ == "__main__":
    main()
