"""Records tests/golden/ikd_nearest.npz from the reference's own ikd-Tree (make_ikd_nearest_golden.md).

    python tests/golden/make_ikd_nearest_golden.py --driver PATH/ikd_nearest_driver [--out FILE]

The driver is the uncommitted program the .md describes: it includes the reference's ikd_Tree.cpp, so
neither its text nor its binary is committed.  This script writes the seeded inputs as job files, runs
the driver on each and packs what the tree answered.
"""
from __future__ import annotations

import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import map_nearest_twin as twin  # noqa: E402

F = np.float32
SEARCHES = [(20, np.inf), (20, 3.0), (20, 0.7), (5, np.inf), (1, np.inf)]  # (k, max_dist)
NQ = 300
BOXES = np.array([[-20, -20, -10, 0, 5, 10], [-5, -10, -10, 15, 10, 10], [30, -50, -2, 50, 50, 2]], F)
# case: seed, built, adds [(n, downsample_on)], ds, delete boxes
CASES = {
    "a": (101, 1400, [], 0.2, None),
    "b": (102, 5000, [(3000, 0)] * 3, 0.2, BOXES),
    "c": (103, 1400, [(3000, 1)], 0.5, None),
}


def cloud(rng, n, ext):
    p = rng.uniform(-ext, ext, (n, 3)).astype(F)
    p[:, 2] *= F(0.1)
    return p


def inputs(case):
    seed, nb, adds, ds, boxes = CASES[case]
    rng = np.random.default_rng(seed)
    built = cloud(rng, nb, 50.0)
    added = [cloud(rng, n, 50.0) for n, _ in adds]
    queries = cloud(rng, NQ, 65.0)  # some lie outside the map
    return built, added, queries


def job(case):
    seed, nb, adds, ds, boxes = CASES[case]
    built, added, queries = inputs(case)
    b = struct.pack("<fI", ds, nb) + built.tobytes() + struct.pack("<I", len(adds))
    for (n, on), pts in zip(adds, added):
        b += struct.pack("<II", n, on) + pts.tobytes()
    nbx = 0 if boxes is None else len(boxes)
    b += struct.pack("<I", nbx) + (b"" if boxes is None else boxes.tobytes())
    b += struct.pack("<I", NQ) + queries.tobytes() + struct.pack("<I", len(SEARCHES))
    for k, md in SEARCHES:
        b += struct.pack("<id", k, md)
    return b


def record(case, driver):
    built, added, queries = inputs(case)
    everything = np.concatenate([built] + added)
    with tempfile.TemporaryDirectory() as tmp:
        jp, rp = os.path.join(tmp, "job.bin"), os.path.join(tmp, "res.bin")
        with open(jp, "wb") as f:
            f.write(job(case))
        subprocess.run([driver, jp, rp], check=True)
        w = np.fromfile(rp, np.uint32)
    ns, valid = int(w[0]), int(w[1])
    assert ns == valid, (ns, valid)  # the all-covering Box_Search returns exactly the valid points
    ids = w[2:2 + ns].astype(np.int64)
    pos = 2 + ns
    store = np.concatenate([everything[ids], ids[:, None].astype(F)], axis=1).astype(F)  # intensity: the original id
    place = np.full(len(everything), -1, np.int64)
    place[ids] = np.arange(ns)
    out = {f"{case}_store": store, f"{case}_queries": queries}
    ties = []
    for s, (k, md) in enumerate(SEARCHES):
        rec = w[pos:pos + NQ * (1 + 2 * k)].reshape(NQ, 1 + 2 * k)
        pos += rec.size
        found = rec[:, 0].astype(np.int32)
        raw = rec[:, 1::2].astype(np.int32)  # original ids, -1 in unused slots
        idx = np.where(raw >= 0, place[np.clip(raw, 0, None)], -1).astype(np.int32)
        assert (idx[raw >= 0] >= 0).all(), "the tree returned a deleted point"
        out[f"{case}_found_{s}"] = found
        out[f"{case}_index_{s}"] = idx
        out[f"{case}_dist_{s}"] = rec[:, 2::2].copy().view(F)
        ties.append(sum(twin.tied(store, q, k) for q in queries))
    assert pos == len(w)
    out[f"{case}_ties"] = np.array(ties, np.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--driver", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "ikd_nearest.npz"))
    a = ap.parse_args()
    data = {"searches_k": np.array([k for k, _ in SEARCHES], np.int32),
            "searches_max_dist": np.array([md for _, md in SEARCHES], np.float64)}
    for case in CASES:
        data.update(record(case, a.driver))
        print(case, "store", len(data[f"{case}_store"]), "ties", data[f"{case}_ties"].tolist())
    np.savez_compressed(a.out, **data)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
