#!/usr/bin/env python3
"""Regroup the rows tests/grad64.py appends to train_parity.jsonl (one per tensor per case) into one line per case:

    python tools/regroup_train_parity.py <dir>/train_parity.jsonl profiles/train_parity.jsonl

A line keeps the case's fields once, and under "tensors" per tensor [e, o32] or [e, o32, o_round] to four significant digits
(ratio = e / o32 and bound = 4 o32 + 2 o_round + 2e-6 follow from them); the analytically zero tensors of grad64.gate_zero go
under "zero" as [max|g|, max|g32|].  Every row must be ok: a run with a failing tensor is not regrouped.  Two tests that name
the same case stay two lines."""
import json
import sys


def sig(x):
    return float(f"{x:.4g}")


def regroup(lines):
    cases, order = {}, []
    for line in lines:
        r = json.loads(line)
        assert r.pop("ok") and r.pop("why") is None, line
        tensor, zero = r.pop("tensor"), r.pop("zero", False)
        fig = [sig(r.pop("e")), sig(r.pop("o32"))] + ([sig(r["o_round"])] if r.get("o_round") else [])
        for k in ("ratio", "bound", "o_round"):
            r.pop(k, None)
        slot, key, n = "zero" if zero else "tensors", json.dumps(r, sort_keys=True), 0
        while (key, n) in cases and tensor in cases[(key, n)].get(slot, {}):
            n += 1
        if (key, n) not in cases:
            cases[(key, n)] = dict(r)
            order.append((key, n))
        cases[(key, n)].setdefault(slot, {})[tensor] = fig
    return [cases[k] for k in order]


if __name__ == "__main__":
    src, dst = sys.argv[1:3]
    with open(src) as f:
        out = regroup(f)
    with open(dst, "w") as f:
        for case in out:
            f.write(json.dumps(case, separators=(",", ":")) + "\n")
    print(f"{len(out)} cases, {sum(len(c.get('tensors', {})) + len(c.get('zero', {})) for c in out)} figures")
