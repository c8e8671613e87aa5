"""Instruction counts of the split-bf16 main loops from a gfx950 assembly listing.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S csrc/gemm_x6.hip -o gemm_x6.s
    python scripts/x6_listing_counts.py gemm_x6.s [--match gemm_x6_kernel] [--full]

For every kernel whose (demangled) name contains --match it finds the main loop (the backward-branch range that
holds the most v_mfma) and counts instructions by category twice: between the first and the last v_mfma of that loop
("span": what issues beside the matrix pipe) and in the rest of the loop body ("rest": the split block of the
unpipelined loops).  --full adds, per v_mfma of the span, the number of VALU instructions up to the next one
(the fillers per gap).  A by-hand check of code generation, not a test.
"""
import argparse
import collections
import re
import subprocess

CATS = [
    ("mfma", r"v_mfma_"),
    ("pk_add_f32", r"v_pk_add_f32"),
    ("pk_mul_f32", r"v_pk_mul_f32"),
    ("pk_fma_f32", r"v_pk_fma_f32"),
    ("cvt_pk_bf16", r"v_cvt_pk_bf16_f32"),
    ("med3", r"v_med3_f32"),
    ("sub/add_f32", r"v_(sub|subrev|add)_f32"),
    ("mul/fma_f32", r"v_(mul|fma|fmac)_f32"),
    ("exp", r"v_exp_f32"),
    ("lshl/and", r"v_(lshlrev_b32|and_b32|and_or_b32|lshl_or_b32|perm_b32|bfi_b32)"),
    ("ds_read", r"ds_read"),
    ("ds_write", r"ds_write"),
    ("vmem", r"(global|buffer|flat)_(load|store|atomic)"),
    ("barrier", r"s_barrier"),
]


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def functions(path):
    """name -> list of instruction / label lines of each .type @function symbol"""
    fns, cur, name = {}, None, None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m and not s.startswith(".L"):
            name, cur = m.group(1), []
            fns[name] = cur
            continue
        if s.startswith(".Lfunc_end") or s.startswith(".section"):
            cur = None
            continue
        if cur is None or not s or s.startswith(";") or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        cur.append(s.split(";")[0].strip())
    return {k: v for k, v in fns.items() if any("v_mfma" in x for x in v)}


def main_loop(ins):
    labels = {x[:-1]: i for i, x in enumerate(ins) if x.endswith(":")}
    best = None
    for i, x in enumerate(ins):
        m = re.match(r"s_cbranch_\w+\s+(\S+)|s_branch\s+(\S+)", x)
        if not m:
            continue
        tgt = m.group(1) or m.group(2)
        j = labels.get(tgt)
        if j is None or j >= i:
            continue
        n = sum("v_mfma" in y for y in ins[j:i])
        if n and (best is None or n > best[0] or (n == best[0] and i - j > best[2] - best[1])):
            best = (n, j, i)
    return ins[best[1]:best[2] + 1] if best else ins


def count(ins):
    c = collections.Counter()
    for x in ins:
        if x.endswith(":"):
            continue
        if x.startswith("v_") and not x.startswith("v_mfma"):
            c["VALU"] += 1
        for name, pat in CATS:
            if re.match(pat, x):
                c[name] += 1
                break
    return c


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("--match", default="")
    ap.add_argument("--full", action="store_true")
    a = ap.parse_args()
    fns = functions(a.listing)
    names = demangle(list(fns))
    for sym, ins in fns.items():
        if a.match and a.match not in names[sym]:
            continue
        loop = main_loop(ins)
        idx = [i for i, x in enumerate(loop) if x.startswith("v_mfma")]
        span, rest = loop[idx[0]:idx[-1] + 1], loop[:idx[0]] + loop[idx[-1] + 1:]
        print(names[sym].replace("(anonymous namespace)::", "").split("(")[0])
        for tag, part in (("span", span), ("rest", rest)):
            c = count(part)
            print(f"  {tag}: VALU {c['VALU']:4d} | " + " ".join(f"{n} {c[n]}" for n, _ in CATS if c[n]))
        if a.full:
            gaps = [sum(x.startswith("v_") for x in loop[p + 1:q]) for p, q in zip(idx, idx[1:])]
            print("  VALU per gap:", " ".join(map(str, gaps)))
