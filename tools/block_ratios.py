#!/usr/bin/env python3
"""Reduce the printed figures of tests/test_gpu_blocks.py (pytest -s) to one line per RUN of the ragged and store-policy cases
(profiles/block_ratios_ragged.txt); the full print is one line per run, precision and tap - 6564 lines for these runs.

    python -m pytest tests/test_gpu_blocks.py -m gpu -s -q > blocks.log
    python tools/block_ratios.py blocks.log > profiles/block_ratios_ragged.txt

bf16 run:  <case[+r<k>]> bf16 taps <n> row <smallest>..<largest device / model ratio> (<tap of the largest>) max <smallest>..<largest>
           (<tap>) exact <largest abs error of the float32-exact taps>
fp32 run:  <case[+r<k>]> fp32 taps <n> abs <largest abs error> (<tap>)       (set k of a case is another list of lengths per precision)
"""
import sys


def main():
    runs = {}
    for line in open(sys.argv[1]):
        if "BLOCKS " not in line or not line.lstrip(".sFEx").startswith("BLOCKS "):   # (pytest's progress marks run into the print)
            continue
        p = line[line.index("BLOCKS "):].split()
        case, prec, tap = p[1], p[2], p[3]
        if "+r" not in case and not case.startswith("pol"):
            continue
        r = runs.setdefault((case, prec), dict(n=0, row=[], max=[], abs=[]))
        r["n"] += 1
        if p[4] == "abs":
            r["abs"].append((float(p[5]), tap))
        else:
            r["row"].append((float(p[6]), tap))
            r["max"].append((float(p[9]), tap))
    print("# tests/test_gpu_blocks.py on the MI355X, ragged runs (<case>+r<k>) and store-policy cases (pol<word>_<case>), one line per run:")
    print("# reduced by tools/block_ratios.py from the printed BLOCKS lines (format in its docstring)")
    for (case, prec), r in runs.items():
        if prec == "fp32":
            print(f"{case} fp32 taps {r['n']} abs {max(r['abs'])[0]:.3e} ({max(r['abs'])[1]})")
        else:
            print(f"{case} bf16 taps {r['n']} row {min(r['row'])[0]:.2f}..{max(r['row'])[0]:.2f} ({max(r['row'])[1]}) "
                  f"max {min(r['max'])[0]:.2f}..{max(r['max'])[0]:.2f} ({max(r['max'])[1]}) exact {max(r['abs'])[0]:.3e}")


if __name__ == "__main__":
    main()
