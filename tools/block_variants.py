#!/usr/bin/env python3
"""Reduce rocprofv3 kernel traces of tests/test_gpu_blocks.py to the list of ConvBlock / EncoderLayer / text-side kernel
instantiations that were launched (profiles/block_variants.txt).

    rocprofv3 --kernel-trace --stats -f csv -d TRACE/main -- python -m pytest tests/test_gpu_blocks.py -m gpu -q -k float64_reference
    rocprofv3 --kernel-trace --stats -f csv -d TRACE/g1 -- python tests/blocks_worker.py /tmp/g1.npz DHW_CHAIN_CONV=3 cases-only
    ...                                                   (the tracer does not follow the test's child processes: one run per static group)
    python tools/block_variants.py TRACE > profiles/block_variants.txt

Notation (tests/blocks_worker.py): cb<BM,CO,NW,OCC,UPC,CH,CIN,TIGHT,PP> = convblock_kernel<bf16, ...> with trailing default template
arguments dropped, a<DM,BM> = enc_a_kernel, bc<DM,BM,NEXT> = enc_bc_kernel, ts<...> / tl<...> = text_style_kernel / text_layer_kernel;
the float32 instantiations carry the prefix "f32:".  tests/test_block_ref_cpu.py compares the list with the case table and with
convblock_init() / enclayer_init().
"""
import csv
import glob
import os
import re
import sys

KINDS = {"convblock_kernel": "cb", "enc_a_kernel": "a", "enc_bc_kernel": "bc", "text_style_kernel": "ts", "text_layer_kernel": "tl"}
CB_DEFAULT = [None, None, None, 1, 0, 0, 0, 0, 0]


def normalise(name):
    m = re.search(r"(convblock_kernel|enc_a_kernel|enc_bc_kernel|text_style_kernel|text_layer_kernel)<(.*?)>\s*\(", name + "(")
    g = re.search(r"\d+(convblock_kernel|enc_a_kernel|enc_bc_kernel|text_style_kernel|text_layer_kernel)I(DF16b|f)((?:Li\d+E)*)E", name)
    if g:   # (the tracer leaves names with the __bf16 type mangled: DF16b)
        kind, f32, ints = KINDS[g.group(1)], g.group(2) == "f", [int(x) for x in re.findall(r"Li(\d+)E", g.group(3))]
    elif m:
        kind, args = KINDS[m.group(1)], [a.strip() for a in m.group(2).split(",")]
        f32 = "float" in args[0] and "bfloat" not in args[0]
        ints = [int(re.sub(r"[^0-9-]", "", a)) for a in args[1:] if re.search(r"\d", a)]
    else:
        return None
    if kind == "cb":
        ints += CB_DEFAULT[len(ints):]
        while len(ints) > 3 and ints[-1] == CB_DEFAULT[len(ints) - 1]:
            ints.pop()
    if kind == "bc" and len(ints) == 2:
        ints.append(0)
    return ("f32:" if f32 else "") + f"{kind}<{','.join(map(str, ints))}>"


def main():
    names = {}
    for root in sys.argv[1:]:
        for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    k = row.get("Kernel_Name") or row.get("Name") or ""
                    names[k] = names.get(k, 0) + 1
    out = {}
    for k, n in names.items():
        v = normalise(k)
        if v:
            out[v] = out.get(v, 0) + n
    if not out:
        sys.exit("no block kernel in the traces: " + "; ".join(sorted(names)[:20]))
    print("# ConvBlock / EncoderLayer / text-side kernel instantiations launched by tests/test_gpu_blocks.py on an MI355X (gfx950),")
    print("# reduced from rocprofv3 --kernel-trace --stats runs by tools/block_variants.py: <instantiation> <dispatches>")
    for v in sorted(out, key=lambda s: (s.startswith("f32:"), s)):
        print(v, out[v])


if __name__ == "__main__":
    main()
