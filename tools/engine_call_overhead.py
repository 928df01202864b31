"""What one Engine wrapper costs in Python, without a GPU: the library is a stand-in whose every export returns 0, so the time of a call
is the wrapper's own staging (pointer views, the memory-space rule, flags, the return-code check, the transfer counters).

    python tools/engine_call_overhead.py                          # this tree: print the record
    python tools/engine_call_overhead.py --parent DIR --store     # ... against the engine.py of a checkout of the parent commit in DIR

10 000 calls each of score_pairs, embed_wave and score_topk over host arrays, 7 repeats, microseconds per call.  With --parent both
modules are loaded into this one process and their repeats alternate (the build host's clock drifts by more than the difference
between two processes), and --store writes both records to profiles/engine_call_ab.json with the verdict: a new median may exceed the
parent's by no more than the parent's own min-to-max spread."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import speakerverification_amd  # noqa: E402,F401  (the package the engine modules below belong to)

CALLS, REPEATS = 10000, 7
STORE = os.path.join(ROOT, "profiles", "engine_call_ab.json")


class NoOpLib:
    def __getattr__(self, name):
        export = lambda *args: 0
        setattr(self, name, export)             # (looked up once: later calls find the attribute)
        return export


def cases_of(root, alias):
    """the three timed calls over the Engine of the checkout at ``root``"""
    spec = importlib.util.spec_from_file_location(f"speakerverification_amd.{alias}", os.path.join(root, "speakerverification_amd", "engine.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    eng = mod.Engine.__new__(mod.Engine)
    eng.lib, eng.h, eng.on_numeric, eng.device, eng._stream = NoOpLib(), None, "raise", 0, None
    eng.embed_dim = 192
    rng = np.random.default_rng(0)
    E, G = rng.standard_normal((3, 192)).astype(np.float32), rng.standard_normal((5, 192)).astype(np.float32)
    ia, ib = np.array([0, 1, 2], np.int32), np.array([1, 2, 0], np.int32)
    wav = rng.standard_normal((3, 800)).astype(np.float32)
    return {"score_pairs": lambda: eng.score_pairs(E, ia, ib), "embed_wave": lambda: eng.embed_wave(wav),
            "score_topk": lambda: eng.score_topk(E, G, 2)}


def measure(builds):
    """builds: {label: cases}; per case the builds' repeats alternate -> {label: {case: record}}"""
    us = {label: {name: [] for name in cases} for label, cases in builds.items()}
    for name in next(iter(builds.values())):
        for cases in builds.values():
            for _ in range(CALLS // 10):
                cases[name]()
        for _ in range(REPEATS):
            for label, cases in builds.items():
                call = cases[name]
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    call()
                us[label][name].append((time.perf_counter() - t0) / CALLS * 1e6)
    return {label: {name: {"repeats_us": r, "median_us": statistics.median(r), "spread_us": max(r) - min(r)} for name, r in per.items()}
            for label, per in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", metavar="DIR", default=None, help="a checkout of the parent commit to alternate with")
    ap.add_argument("--store", action="store_true", help="with --parent: write both records to profiles/engine_call_ab.json")
    args = ap.parse_args()
    builds = {"parent": cases_of(args.parent, "engine_parent")} if args.parent else {}
    builds["new"] = cases_of(ROOT, "engine_new")
    record = measure(builds)
    if args.parent:
        record["new_median_within_parent_median_plus_spread"] = {
            k: v["median_us"] <= record["parent"][k]["median_us"] + record["parent"][k]["spread_us"] for k, v in record["new"].items()}
    print(json.dumps(record, indent=1))
    if args.store and args.parent:
        doc = json.load(open(STORE)) if os.path.exists(STORE) else {}
        doc["python_per_call"] = {"what": f"{CALLS} calls per repeat over a no-op library and host arrays, {REPEATS} repeats alternating between the two "
                                          "engine.py in one process, microseconds per call, on the build host's CPU", **record}
        with open(STORE, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
