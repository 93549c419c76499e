"""Writes wgrad_bits.json: per case of tests/test_gpu_wgrad_bits.py, the sha256 of the raw bytes of dW and of db that THIS
checkout's build computes on the GPU, with the commit it was run at.

Run it at the commit the record is to be of (a clean checkout whose library is built), never to make a failing test pass: the test names
the commit and holds the kernels to its bits.

    python tests/golden/make_wgrad_bits.py [--commit HASH] [--out tests/golden/wgrad_bits.json]

--commit: the checkout's commit when it is not a git work tree (default: git rev-parse HEAD).  Every case is run through the
test's own run_case, so a digest is recorded only of a result that passed the f64 restatement and the plan's slice count.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit")
    ap.add_argument("--out", default=os.path.join(HERE, "wgrad_bits.json"))
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    import torch
    import test_gpu_wgrad_bits as T
    assert torch.cuda.is_available(), "needs a HIP device"
    cases = {}
    for kind, name in T.ALL:
        dw, db = T.run_case("cuda:0", kind, name)
        cases[f"{kind}/{name}"] = {"dw": T.digest(dw), "db": T.digest(db)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"parent_commit": commit, "cases": cases}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(cases)} cases at {commit} -> {args.out}")


if __name__ == "__main__":
    main()
