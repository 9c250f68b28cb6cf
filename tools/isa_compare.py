"""Kernel-by-kernel comparison of two builds' gfx950 assembly (the `*gfx950*.s` files that
`hipcc --save-temps -c` leaves behind), for refactors that must not change the generated code.

    python tools/isa_compare.py --old DIR --new DIR --out profiles/NAME.json [--brief] [--added REGEX] [--dropped REGEX]

One row per kernel, one line each: old and new name, the code-object notes (VGPR / AGPR / SGPR counts,
spills, private segment and LDS bytes), the instruction count and a SHA-256 of the instructions with symbol names and
label numbers normalised.  Counts and hashes only — no instruction text.  Exit status 1 when the kernel
sets do not match one to one or a kernel's notes differ.  --added REGEX: kernels only the new build has whose
name matches (new template instances) are listed under "added" with their notes instead of counting as a mismatch;
--dropped REGEX: the same for kernels only the old build has (removed kernels), listed under "dropped".
"""
from __future__ import annotations

import argparse
import hashlib
import json
import re
import shutil
import subprocess
import sys
from pathlib import Path

NOTES = {"vgpr": ".vgpr_count", "agpr": ".agpr_count", "sgpr": ".sgpr_count", "vgpr_spill": ".vgpr_spill_count",
         "sgpr_spill": ".sgpr_spill_count", "private_segment": ".private_segment_fixed_size",
         "lds": ".group_segment_fixed_size"}

# (pattern, replacement) pairs: old demangled kernel name -> its new name, for a refactor that renames kernels or
# adds template arguments, e.g. (re.compile(r"(k_name<[^<>]*)>"), r"\1, false>").  Empty: names pair as they are.
RENAMES = []


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def kernels_of(asm: str):
    """{mangled name: row} of one assembly file."""
    rows = {}
    meta = asm[asm.index("amdhsa.kernels:"):asm.index("amdhsa.target:")]
    for item in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", item).group(1)
        rows[name] = {k: int(re.search(re.escape(key) + r":\s+(\d+)", item).group(1)) for k, key in NOTES.items()}
    for name, row in rows.items():
        body = asm[asm.index(f"\n{name}: "):]
        body = body[:re.search(r"\n\.Lfunc_end\d+:", body).start()]
        labels, ins = {}, []
        for line in body.splitlines()[2:]:  # (after the kernel's own label)
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") and not line.endswith(":"):
                continue
            line = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), f"L{len(labels)}"), line)
            line = re.sub(r"\b_Z\w+", "SYM", line)
            ins.append(line)
        row["instructions"] = sum(1 for l in ins if not l.endswith(":"))
        row["sha256"] = hashlib.sha256("\n".join(ins).encode()).hexdigest()
    return rows


def load(d: Path):
    rows = {}
    for f in sorted(d.rglob("*gfx950*.s")):
        rows.update(kernels_of(f.read_text()))
    dm = demangle(list(rows))
    return {dm[n].split("(")[0]: dict(row, name=n) for n, row in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", type=Path, required=True)
    ap.add_argument("--new", type=Path, required=True)
    ap.add_argument("--out", type=Path, required=True)
    ap.add_argument("--brief", action="store_true",
                    help="a kernel whose notes, count and hash are all equal gets the row [name, instructions, sha256[:16]]")
    ap.add_argument("--added", default=None, metavar="REGEX",
                    help="kernels only the new build has are listed, not problems, where their name matches")
    ap.add_argument("--dropped", default=None, metavar="REGEX",
                    help="kernels only the old build has are listed, not problems, where their name matches")
    a = ap.parse_args()
    old, new = load(a.old), load(a.new)
    table, bad, dropped, cols = [], [], {}, (*NOTES, "instructions", "sha256")
    for dname, o in sorted(old.items()):
        nname = dname
        for pat, rep in RENAMES:
            nname = pat.sub(rep, nname)
        n = new.pop(nname, None)
        if n is None:
            if a.dropped and re.search(a.dropped, dname):
                dropped[dname] = [o[k] for k in cols[:-1]]
            else:
                bad.append(f"dropped: {dname}")
            continue
        notes_equal = all(o[k] == n[k] for k in NOTES)
        if not notes_equal:
            bad.append(f"notes differ: {dname}: " + ", ".join(f"{k} {o[k]}->{n[k]}" for k in NOTES if o[k] != n[k]))
        table.append({"kernel": dname, "old_name": o["name"], "new_name": n["name"] if nname != dname else None,
                      "old": [o[k] for k in cols], "new": [n[k] for k in cols] if o != dict(n, name=o["name"]) else None,
                      "hash_equal": o["sha256"] == n["sha256"]})
    added = sorted(d for d in new if a.added and re.search(a.added, d))
    bad += [f"added: {d}" for d in new if d not in added]
    differ = [r["kernel"] for r in table if not r["hash_equal"]]
    # one row per line; new_name / new are null where they equal old_name / old
    head = {"kernels": len(table), "problems": bad, "hash_differs": len(differ), "columns": cols}
    if added:
        head["added"] = {d: [new[d][k] for k in cols[:-1]] for d in added}
    if dropped:
        head["dropped"] = dropped
    lines = [json.dumps(r) for r in table]
    if a.brief:   # equal kernels first, four to a line; then the full rows of the rest
        same = [r for r in table if r["new"] is None and r["new_name"] is None]
        short = [json.dumps([r["kernel"], r["old"][-2], r["old"][-1][:16]]) for r in same]
        lines = [", ".join(short[i:i + 4]) for i in range(0, len(short), 4)] + [json.dumps(r) for r in table if r not in same]
    a.out.write_text("{" + json.dumps(head)[1:-1] + ',\n"rows": [\n' + ",\n".join(lines) + "\n]}\n")
    print(f"{len(table)} kernels matched, {len(differ)} differ in hash, {len(dropped)} dropped as expected, "
          f"{len(bad)} problems")
    for b in bad:
        print("  " + b)
    for d in differ:
        print("  hash differs: " + d)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
