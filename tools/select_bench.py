#!/usr/bin/env python3
"""Timings of the all-candidates scan under a field selection (pf_set_scan_select) at full size:
one-query scan_keys_async steps on a caller's stream, as bench.py's cfg 2 runs them, over the seeded
1,632,803-user corpus, with no selection, text only (no fixed field), fixed only (no column) and
one column (the one holding the most tokens, no fixed field).  Each run is a child process of its
own.  With --parent-root DIR (a built checkout of the parent commit) the parent's unselected steps
for the same queries are timed in alternation with this tree's, so both see the same machine; the
parent's tree is only asked for what it has.  The first child of this tree also measures what the
selection replaces for a caller of the C++ facade, a second engine on the same corpus: the wall
time of a second pf_open and the device memory it takes (the free-memory difference around it).
Reported, not gated.

    python tools/select_bench.py [--users N --steps K --warmup W --rounds R --parent-root DIR --out FILE --commit ID]

Reads nothing outside the repository (and DIR); writes FILE (default profiles/fsel_select_bench.json)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPK = 10


def child(args):
    root = os.path.abspath(args.root or ROOT)
    sys.path.insert(0, os.path.join(root, "recommendation-system-pokec_amd"))
    sys.path.insert(0, os.path.join(root, "tools"))
    sys.path.insert(0, os.path.join(root, "tests"))
    import synth
    import torch
    import pokec_fas as pf
    corpus = synth.Corpus(n_users=args.users, seed=1, edge_cases=0, threads=16)
    desc = corpus.desc_ptr()
    t = time.perf_counter()
    eng = pf.FasEngine(desc, 0)
    open_s = time.perf_counter() - t
    kernel = eng.layout().scan_kernel
    rng = np.random.default_rng(2)  # bench.py's cfg-2 query stream
    qs = rng.integers(1, args.users + 1, size=(args.warmup + args.steps, 1)).astype(np.int32)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sptr = stream.cuda_stream
    keys = torch.empty((args.warmup + args.steps, TOPK), dtype=torch.int64, device="cuda")

    def timed(sel):
        if sel is not None:
            eng.set_scan_select(sel)
        for i in range(args.warmup):
            eng.scan_keys_async(qs[i], TOPK, keys[i].data_ptr(), sptr)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.warmup, args.warmup + args.steps):
            eng.scan_keys_async(qs[i], TOPK, keys[i].data_ptr(), sptr)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        if sel is not None:
            eng.clear_scan_select()
        return ms

    rows = [{"select": "none", "fixed": None, "cols": None, "ms_per_step": timed(None)}]
    out = {"tree": "parent" if args.unselected_only else "this", "scan_kernel": "K5" if kernel == 2 else "K1",
           "users": args.users, "steps": args.steps, "warmup": args.warmup, "topk": TOPK, "first_open_s": open_s}
    if not args.unselected_only:
        import pokec_testlib as tl
        d = tl.PfCorpusDesc.from_address(desc)
        T = d.n_cols
        off = np.ctypeslib.as_array(ctypes_ptr(d.tok_off), shape=(d.n_users * T + 1,))
        per_col = np.diff(off).reshape(d.n_users, T).sum(axis=0)
        big = int(per_col.argmax())
        S = pf.FieldSelect.make
        for name, sel in (("text_only", S(fixed=0)), ("fixed_only", S(cols=0)), ("one_column", S(fixed=0, cols=[big]))):
            rows.append({"select": name, "fixed": int(sel.fixed), "cols": "%x" % (int(sel.cols) & ((1 << T) - 1)),
                         "ms_per_step": timed(sel)})
        rows.append({"select": "none_again", "fixed": None, "cols": None, "ms_per_step": timed(None)})
        out["one_column"] = {"column": big, "tokens": int(per_col[big]), "all_tokens": int(per_col.sum()), "n_cols": T}
        if args.second_open:  # what the facade's second engine costs: once
            torch.cuda.synchronize()
            free0, total = torch.cuda.mem_get_info()
            t0 = time.perf_counter()
            eng2 = pf.FasEngine(desc, 0)
            dt = time.perf_counter() - t0
            torch.cuda.synchronize()
            free1, _ = torch.cuda.mem_get_info()
            out["second_engine"] = {"pf_open_s": dt, "hbm_bytes": int(free0 - free1), "hbm_total_bytes": int(total)}
            eng2.close()
    out["rows"] = rows
    eng.close()
    print("result " + json.dumps(out), flush=True)


def ctypes_ptr(addr):
    import ctypes
    return ctypes.cast(addr, ctypes.POINTER(ctypes.c_int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1632803)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of (parent, this tree)")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsel_select_bench.json"))
    ap.add_argument("--commit", default="unknown", help="the parent commit the tree was measured against")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=None, help="(child) the tree whose engine is measured")
    ap.add_argument("--unselected-only", action="store_true", help="(child) a tree without pf_set_scan_select")
    ap.add_argument("--second-open", action="store_true", help="(child) also time a second pf_open")
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    for r in range(args.rounds):
        for tree in (("parent", "this") if args.parent_root else ("this",)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--users", str(args.users), "--steps", str(args.steps),
                   "--warmup", str(args.warmup)]
            if tree == "parent":
                cmd += ["--root", args.parent_root, "--unselected-only"]
            elif r == 0:
                cmd += ["--second-open"]
            p = subprocess.run(cmd, env={**os.environ, "PF_LIB_PATH": ""}, capture_output=True, text=True, timeout=1100)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("result ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout + p.stderr)
                return 1
            runs.append(json.loads(line[0][7:]))
            print(json.dumps(runs[-1]), flush=True)
    res = {"tool": "tools/select_bench.py", "parent_commit": args.commit,
           "what": "one-query scan_keys_async steps (cfg 2's step) under field selections; ms per step, host clock over the "
                   "timed steps; parent and this tree in alternation, one child process each; second_engine = a second "
                   "pf_open on the same corpus in the first child of this tree",
           "runs": runs}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
