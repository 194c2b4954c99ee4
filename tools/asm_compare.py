#!/usr/bin/env python3
"""Compare the gfx950 assembly of two trees, kernel by kernel.

    tools/asm_compare.py OLD_TREE NEW_TREE [--diff] [--only FILE]

Every file of __graft_entry__.HIP_SRC is compiled in both trees, device only,
to assembly, with __graft_entry__.HIP_FLAGS less what belongs to the host link.
Comment lines and trailing comments, .ident, .file and the __hip_cuid_* symbol
are stripped (they carry the compiler's build and a hash of the source path).
Per kernel, three texts are compared: the function's body, its .amdhsa_kernel
descriptor and its entry in the code object's metadata.  A row says identical
or not and gives, old / new: instructions, VGPRs, SGPRs, LDS bytes, scratch
bytes.  What a file holds outside its kernels is one more row.  For a kernel
that differs the row is followed by whether the instruction count per mnemonic
is equal and, with --diff, by the differing lines.

The exit status is 0 if everything is identical, 1 if anything differs, 2 if a
file did not compile.  Needs hipcc and no GPU; at most 16 compilers run at once.
"""
import argparse
import collections
import concurrent.futures
import difflib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as entry  # noqa: E402

HOST_LINK = ("-shared", "-fPIC")
FIGURES = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"),
           ("scratch", ".private_segment_fixed_size"))


def device_flags():
    return [f for f in entry.HIP_FLAGS if f not in HOST_LINK and not f.startswith("-Wl,")]


def compile_asm(tree, rel, out):
    cmd = [entry.HIPCC, *device_flags(), "--cuda-device-only", "-S", "-I", os.path.join(tree, "include"), "-o", out,
           os.path.join(tree, rel)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


def strip(text):
    """The assembly without what differs from build to build."""
    out = []
    meta = False  # inside the code object's metadata: YAML, its indentation kept
    for line in text.splitlines():
        s = line.rstrip() if meta else line.strip()
        if s.strip() in (".amdgpu_metadata", ".end_amdgpu_metadata"):
            meta = s.strip() == ".amdgpu_metadata"
        if not s.startswith((".asci", ".string")):  # (a string may hold a ';')
            s = s.split(";", 1)[0].rstrip()
        if not s or s.startswith((".ident", ".file")) or "__hip_cuid_" in s:
            continue
        out.append(s)
    return out


def split_kernels(lines):
    """{kernel: {"body", "desc", "meta": [lines], figures...}} and the lines outside all of them."""
    names = [ln.split()[1] for ln in lines if ln.startswith(".amdhsa_kernel ")]
    kernels = {n: {"body": [], "desc": [], "meta": []} for n in names}
    rest = []
    cur = part = None
    for ln in lines:
        if cur is None:
            if ln.endswith(":") and ln[:-1] in kernels:
                cur, part = ln[:-1], "body"
            elif ln.startswith(".amdhsa_kernel "):
                cur, part = ln.split()[1], "desc"
            elif ln.startswith("  - ."):
                cur, part = "?", "meta"  # named by its .name line below
                pending = [ln]
            else:
                rest.append(ln)
            continue
        if part == "body":
            if ln.startswith(".Lfunc_end") and ln.endswith(":"):
                cur = None
            else:
                kernels[cur]["body"].append(ln)
        elif part == "desc":
            if ln == ".end_amdhsa_kernel":
                cur = None
            else:
                kernels[cur]["desc"].append(ln)
        else:  # one kernel's metadata entry: up to the next entry or the end of the list
            if not ln.startswith("    "):
                name = next((p.split(":", 1)[1].strip() for p in pending if p.startswith("    .name:")), None)
                if name in kernels:
                    kernels[name]["meta"] = pending
                else:
                    rest.extend(pending)
                if ln.startswith("  - ."):
                    pending = [ln]
                else:
                    cur = None
                    rest.append(ln)
            else:
                pending.append(ln)
    for k in kernels.values():
        k["insts"] = [ln for ln in k["body"] if not ln.startswith(".") and not ln.endswith(":")]
        for key, field in FIGURES:
            k[key] = next((ln.split(":", 1)[1].strip() for ln in k["meta"] if ln[4:].startswith(field + ":")), "?")
    return kernels, rest


def mnemonics(insts):
    return collections.Counter(ln.split()[0] for ln in insts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--diff", action="store_true", help="print the differing lines of what differs")
    ap.add_argument("--only", metavar="FILE", action="append", help="compare this file of HIP_SRC only (repeatable)")
    args = ap.parse_args()
    rels = [os.path.relpath(p, entry.ROOT) for p in entry.HIP_SRC]
    if args.only:
        rels = [r for r in rels if os.path.basename(r) in args.only]
    tmp = tempfile.TemporaryDirectory(prefix="asm_compare_")
    work = tmp.name
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        for side, tree in (("old", args.old_tree), ("new", args.new_tree)):
            os.makedirs(os.path.join(work, side), exist_ok=True)
            for rel in rels:
                out = os.path.join(work, side, os.path.basename(rel) + ".s")
                jobs[side, rel] = (out, pool.submit(compile_asm, os.path.abspath(tree), rel, out))
    failed = False
    for (side, rel), (out, fut) in jobs.items():
        rc, log = fut.result()
        if rc != 0:
            failed = True
            print(f"{side} {rel}: hipcc failed\n{log}", file=sys.stderr)
    if failed:
        return 2

    differ = 0
    print(f"{'file':16} {'kernel':76} {'same':5} {'insts':>13} {'vgpr':>9} {'sgpr':>9} {'lds':>13} {'scratch':>9}")
    for rel in rels:
        sides = {}
        for side in ("old", "new"):
            with open(jobs[side, rel][0]) as f:
                sides[side] = split_kernels(strip(f.read()))
        (ok, orest), (nk, nrest) = sides["old"], sides["new"]
        name = os.path.basename(rel)

        def short(kern):  # (a library's kernels carry their whole configuration in the name)
            return kern if len(kern) <= 76 else kern[:60] + "..." + kern[-13:]

        for kern in list(ok) + [k for k in nk if k not in ok]:
            o, n = ok.get(kern), nk.get(kern)
            if o is None or n is None:
                differ += 1
                print(f"{name:16} {short(kern):76} {'only in ' + ('old' if n is None else 'new')}")
                continue
            same = all(o[p] == n[p] for p in ("body", "desc", "meta"))
            differ += not same

            def pair(key):
                a, b = (len(o[key]), len(n[key])) if key == "insts" else (o[key], n[key])
                return f"{a}/{b}"

            print(f"{name:16} {short(kern):76} {'yes' if same else 'NO':5} {pair('insts'):>13} {pair('vgpr'):>9} "
                  f"{pair('sgpr'):>9} {pair('lds'):>13} {pair('scratch'):>9}")
            if same:
                continue
            om, nm = mnemonics(o["insts"]), mnemonics(n["insts"])
            if om == nm:
                print(f"{'':16}   instruction count per mnemonic: equal")
            else:
                delta = ", ".join(f"{m} {om[m]}->{nm[m]}" for m in sorted(set(om) | set(nm)) if om[m] != nm[m])
                print(f"{'':16}   instruction count per mnemonic: differs ({delta})")
            if args.diff:
                for part in ("body", "desc", "meta"):
                    for ln in difflib.unified_diff(o[part], n[part], f"old {kern} {part}", f"new {kern} {part}",
                                                   n=0, lineterm=""):
                        print("    " + ln)
        same = orest == nrest
        differ += not same
        print(f"{name:16} {'(outside the kernels)':76} {'yes' if same else 'NO':5}")
        if not same and args.diff:
            for ln in difflib.unified_diff(orest, nrest, "old", "new", n=0, lineterm=""):
                print("    " + ln)
    print(f"{differ} of the rows differ" if differ else "all identical")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
