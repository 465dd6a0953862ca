#!/usr/bin/env python3
"""Are two sets of device assembly files the same code, function by function?

For a kernel refactor that must not change device code: compile the old and the new translation
units with the library's HIPFLAGS plus `--cuda-device-only -S` and compare.

    python scripts/kernel_isa_diff.py old.s [old2.s ...] -- new1.s new2.s ...

Every function (symbol line to its .Lfunc_end) is taken with comments stripped and the function
index dropped from its .LBB<n>_ / .Ltmp<n> labels, and every kernel's .amdhsa_kernel block (VGPRs,
SGPRs, scratch, LDS) as it stands.  Passes if both sides hold the same names with identical text;
a name may repeat on one side only with identical text, and only a non-kernel (an inline device
function emitted by each file that uses it).  Exit status 1 otherwise."""
import re
import sys
from pathlib import Path


def functions(path):
    """{name: normalised text} and {kernel: descriptor block} of one assembly file."""
    funcs, descs, cur, name, is_function = {}, {}, None, None, set()
    for raw in Path(path).read_text().splitlines():
        line = re.sub(r"\s*;.*$", "", raw).rstrip()
        m = re.match(r"^\s*\.type\s+([\w$.]+),@function$", line)
        if m:
            is_function.add(m.group(1))
        m = re.match(r"^([A-Za-z_][\w$.]*):$", line)
        if m and cur is None and m.group(1) in is_function:
            name, cur = m.group(1), []
        if cur is None or not line:
            continue
        cur.append(re.sub(r"\.L(BB|tmp|func_end|func_begin)\d+", r".L\1", line))
        if line.lstrip().startswith(".amdhsa_kernel "):  # the descriptor lies inside the function's span
            dstart = len(cur) - 1
        elif line.lstrip().startswith(".end_amdhsa_kernel"):
            descs[name] = "\n".join(cur[dstart:])
        elif cur[-1] == ".Lfunc_end:":
            assert name not in funcs, (path, name)
            funcs[name], cur = "\n".join(cur), None
    return funcs, descs


def side(paths):
    funcs, descs, where = {}, {}, {}
    for p in paths:
        f, d = functions(p)
        for n, text in f.items():
            where.setdefault(n, []).append(p)
            if n in funcs and (funcs[n] != text or n in d):
                print(f"DIFFERENT COPIES / REPEATED KERNEL {n}: {where[n]}")
                sys.exit(1)
            funcs[n] = text
        descs.update(d)
    return funcs, descs, where


def main():
    k = sys.argv.index("--")
    old_f, old_d, _ = side(sys.argv[1:k])
    new_f, new_d, where = side(sys.argv[k + 1:])
    bad = 0
    for title, old, new in (("function", old_f, new_f), ("kernel descriptor", old_d, new_d)):
        for n in sorted(set(old) | set(new)):
            if n not in old or n not in new:
                print(f"{title} only {'old' if n in old else 'new'}: {n}")
                bad += 1
            elif old[n] != new[n]:
                print(f"{title} differs: {n}")
                bad += 1
    repeated = sorted(n for n, w in where.items() if len(w) > 1)
    print(f"{len(old_f)} functions ({len(old_d)} kernels) old, {len(new_f)} ({len(new_d)}) new in "
          f"{len(sys.argv) - k - 1} files; {bad} differences; emitted by several files: {repeated}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
