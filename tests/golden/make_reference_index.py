#!/usr/bin/env python3
"""Generates tests/golden/reference_index.json: the facts about the reference (the Rust fhe.rs checkout the patches of
rust/patches/ target) that tests/test_rust_shim.py and tests/test_oracle_rq_bfv.py check against, so that the suite
needs no reference checkout.  The file holds data only -- line hashes, identifier names and visibilities, counts,
constants -- never source text.

    python tests/golden/make_reference_index.py <reference checkout>   # rewrites the fixture in place

Entries:
  rq_moduli             the `MODULI` constant of crates/fhe-math/src/rq/mod.rs (its tests' moduli)
  patch_targets         per file a patch touches: null when the reference does not have it, else {line number: the first
                        12 hex digits of the SHA-256 of that line (newline stripped)} for the lines the hunks use as
                        context -- enough to check that every hunk's context stands where the hunk says, as
                        `patch --dry-run` does (tests/test_rust_shim.py: test_patches_apply_to_the_reference)
  fn_names              every `fn <name>` defined under crates/
  fields / methods      name -> [[visibility, file]] of struct fields and fns outside #[cfg(test)] (trait methods count
                        as `pub`); file is relative to the checkout, crates/<crate>/...
  struct_literals       per patch target: for Context / Scaler / KeySwitchingKey / Multiplicator, how many struct
                        literals (`Self {` or `<Owner> {` opening a line) its non-test code holds
  bfv_bench_strings     the one-word string literals of crates/fhe/benches/bfv.rs (its Criterion IDs)
Before writing, every patch is dry-run against the checkout with `patch`, so the fixture is only made from a reference
the patches really apply to."""
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATCH_DIR = os.path.join(ROOT, "rust", "patches")
OUT = os.path.join(ROOT, "tests", "golden", "reference_index.json")
OWNERS = ("Context", "Scaler", "KeySwitchingKey", "Multiplicator")


def line_hash(line):
    return hashlib.sha256(line.encode()).hexdigest()[:12]


def file_hunks(text):
    """[(target, creates the file, [(old start line, [old-side lines])])] of a unified diff: per file, every hunk's
    context and removed lines -- what must stand in the target for the hunk to apply."""
    lines, files, i = text.split("\n"), [], 0
    while i < len(lines):
        if lines[i].startswith("+++ "):
            target = None if lines[i].startswith("+++ /dev/null") else lines[i][6:]
            files.append((target, lines[i - 1].startswith("--- /dev/null"), []))
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+\d+(?:,(\d+))? @@", lines[i])
        i += 1
        if not m:
            continue
        n_old, n_new, old = int(m.group(2) or 1), int(m.group(3) or 1), []
        while n_old > 0 or n_new > 0:
            line = lines[i]
            i += 1
            if line.startswith("\\"):
                continue
            tag = line[:1] or " "
            if tag in " -":
                old.append(line[1:])
                n_old -= 1
            if tag in " +":
                n_new -= 1
        files[-1][2].append((int(m.group(1)), old))
    return files


def place_hunks(hunks, hashes):
    """The line (1-based) at which each hunk's old-side lines stand in a file given as {line number: line hash}: in
    order, without fuzz, the match nearest the line the hunk states (as `patch` takes it).  None when one does not apply."""
    pos, at = 1, []
    for start, old in hunks:
        want = [line_hash(l) for l in old]
        cand = [k for k in sorted(hashes) if k >= pos and all(hashes.get(k + j) == w for j, w in enumerate(want))]
        if not cand:
            return None
        at.append(min(cand, key=lambda k: abs(k - start)))
        pos = at[-1] + len(want)
    return at


def patches():
    """{patch file name: file_hunks(its text)} of rust/patches/."""
    return {f: file_hunks(open(os.path.join(PATCH_DIR, f)).read())
            for f in sorted(os.listdir(PATCH_DIR)) if f.endswith(".patch")}


def items(ref):
    """fields / methods: name -> [[visibility, file]] over the reference's crates (non-test code)."""
    fields, methods = {}, {}
    for base, _, files in sorted(os.walk(os.path.join(ref, "crates"))):
        for fn in sorted(files):
            if not fn.endswith(".rs"):
                continue
            path = os.path.join(base, fn)
            rel = os.path.relpath(path, ref)
            src = open(path).read().split("#[cfg(test)]")[0]
            for sm in re.finditer(r"pub(?:\([a-z]+\))? struct \w+(?:<[^>]*>)? \{(.*?)\n\}", src, flags=re.S):
                for fm in re.finditer(r"^\s*(pub(?:\((?:crate|super)\))? )?([a-z_][a-z0-9_]*):", sm.group(1), flags=re.M):
                    vis = (fm.group(1) or "").strip() or "private"
                    fields.setdefault(fm.group(2), []).append([vis, rel])
            # methods of a trait (declared in `pub trait T {` or implemented in `impl T for X {`) carry no `pub`: they are
            # as visible as the trait, which for every trait of these crates' APIs is public
            trait_spans = []
            for tm in re.finditer(r"^(?:pub trait \w+[^{;]*|impl(?:<[^>]*>)? [\w:<>, &']+ for [^{;]+)\{", src, flags=re.M):
                depth, i = 1, tm.end()
                while i < len(src) and depth:
                    depth += {"{": 1, "}": -1}.get(src[i], 0)
                    i += 1
                trait_spans.append((tm.end(), i))
            for mm in re.finditer(r"^\s*(pub(?:\((?:crate|super)\))? )?(?:const )?(?:unsafe )?fn ([a-z_][a-z0-9_]*)", src, flags=re.M):
                vis = (mm.group(1) or "").strip() or "private"
                if vis == "private" and any(a <= mm.start() < b for a, b in trait_spans):
                    vis = "pub"
                methods.setdefault(mm.group(2), []).append([vis, rel])
    return fields, methods


def struct_literals(src):
    body = src.split("#[cfg(test)]")[0]
    return {owner: len(re.findall(r"(?<!-> )\b(?:Self|%s) \{\n" % owner, body))
            - len(re.findall(r"pub struct %s \{\n" % owner, body))
            - len(re.findall(r"impl(?:<[^>]*>)? (?:\w+(?:<[^>]*>)? for )?%s \{\n" % owner, body))
            for owner in OWNERS}


def main(ref):
    for f in sorted(os.listdir(PATCH_DIR)):
        if f.endswith(".patch"):
            subprocess.run(["patch", "--dry-run", "-p1", "-s", "-i", os.path.join(PATCH_DIR, f)], cwd=ref, check=True)
    rq = open(os.path.join(ref, "crates", "fhe-math", "src", "rq", "mod.rs")).read()
    m = re.search(r"const MODULI: &\[u64; 5\] = &\[(.*?)\];", rq, re.S)
    targets, literals = {}, {}
    for f, files in patches().items():
        for t, _, hunks in files:
            p = os.path.join(ref, t)
            if not os.path.exists(p):
                targets[t] = None
                continue
            src = open(p).read()
            every = {n + 1: line_hash(l) for n, l in enumerate(src.split("\n"))}
            at = place_hunks(hunks, every)
            assert at is not None, (f, t)
            kept = targets.setdefault(t, {})
            for k, (_, old) in zip(at, hunks):
                kept.update({k + j: every[k + j] for j in range(len(old))})
            if t.endswith(".rs"):
                literals[t] = struct_literals(src)
    fn_names = set()
    for base, _, files in os.walk(os.path.join(ref, "crates")):
        for fn in files:
            if fn.endswith(".rs"):
                fn_names.update(re.findall(r"\bfn ([a-z_][a-z0-9_]*)", open(os.path.join(base, fn)).read()))
    fields, methods = items(ref)
    bench = open(os.path.join(ref, "crates", "fhe", "benches", "bfv.rs")).read()
    index = dict(rq_moduli=[int(x) for x in re.findall(r"\d+", m.group(1))], patch_targets=targets,
                 fn_names=sorted(fn_names), fields=fields, methods=methods, struct_literals=literals,
                 bfv_bench_strings=sorted(set(re.findall(r'"([\w{}=/()]+)"', bench))))
    # one line per entry of each table
    with open(OUT, "w") as f:
        entries = []
        for k in sorted(index):
            v = index[k]
            if isinstance(v, dict):
                rows = ",\n".join(" %s: %s" % (json.dumps(str(kk)), json.dumps(v[kk], sort_keys=True)) for kk in sorted(v))
                entries.append("%s: {\n%s\n}" % (json.dumps(k), rows))
            else:
                entries.append("%s: %s" % (json.dumps(k), json.dumps(v)))
        f.write("{\n" + ",\n".join(entries) + "\n}\n")
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
