#!/usr/bin/env python3
"""Records cull_table_digests.json: the digests of tests/native/cull_tables_digest_main.cpp for the table builder of ONE
commit, which a later change of the builder that must not move a byte of the tables is then held against
(tests/test_cull_tables_digest_host.py).

    python tests/golden/make_cull_table_digests.py --rev <commit>

The builder's sources (pt_scene.hpp, pt_scene.cpp and, where the commit has it, pt_cull_tables.cpp) are taken from that
commit with `git show` into a scratch directory; the digest program is today's.  The test-hook build is run with g++ -O0,
g++ -O2 and (where it exists) ROCm's clang++ -O3, all without contraction, and the plain build with g++ -O2: the file is
written only if every build agrees on every case, so the recorded digests do not depend on the compiler.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import test_cull_tables_digest_host as T

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", required=True, help="the commit whose table builder is recorded")
    a = ap.parse_args()
    repo = os.path.dirname(ROOT)
    rev = subprocess.check_output(["git", "-C", repo, "rev-parse", a.rev], text=True).strip()
    with tempfile.TemporaryDirectory() as tmp:
        csrc = os.path.join(tmp, "csrc")
        os.makedirs(csrc)
        for f in ("pt_scene.hpp", "pt_scene.cpp", "pt_cull_tables.cpp"):
            show = subprocess.run(["git", "-C", repo, "show", f"{rev}:path-tracing_amd/csrc/{f}"], capture_output=True, text=True)
            if show.returncode == 0:
                open(os.path.join(csrc, f), "w").write(show.stdout)
        replicas = T.make_replicas(tmp)
        compilers = [("g++", "-O0"), ("g++", "-O2")] + ([(CLANG, "-O3")] if os.path.exists(CLANG) else [])
        runs = {}
        for k, comp in enumerate(compilers):
            exe = T.build_digest_program(os.path.join(tmp, f"digest{k}"), True, csrc, comp)
            runs[" ".join(comp).replace(CLANG, "ROCm clang++")] = T.run_digest_program(exe, replicas)
        plain = T.run_digest_program(T.build_digest_program(os.path.join(tmp, "digest_plain"), False, csrc), replicas)
    digests = runs["g++ -O2"]
    for name, got in runs.items():
        assert got == digests, (name, {k: (got.get(k), v) for k, v in digests.items() if got.get(k) != v})
    assert plain == {k: v for k, v in digests.items() if not k.startswith("hooks:")}, "the hook build at default knobs differs from the plain build"
    out = os.path.join(HERE, "cull_table_digests.json")
    json.dump({"recorded_from_commit": rev, "agreeing_builds": sorted(runs) + ["g++ -O2 (no hooks)"], "digests": digests}, open(out, "w"), indent=1)
    open(out, "a").write("\n")
    print(f"wrote {out}: {len(digests)} cases from {rev}, identical under {', '.join(runs)}")


if __name__ == "__main__":
    main()
