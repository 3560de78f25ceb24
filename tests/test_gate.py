"""Doppler-gated registration, the parts that need no GPU (include/icp4r/icp4r_gate.h): the ABI of the
new header, and icp4r_sequence_pairs — pure host code — against the node's literal accumulate-and-clear
loop (tests/gate_twin.py), with the two bounds the rule implies: a registered target holds at most one
non-empty scan and a registered source at most two.  tests/cpp/gate_host_check.cpp runs the same host
code under ASan + UBSan as a stand-alone program."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import gate_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE_HEADER = os.path.join(ROOT, "include", "icp4r", "icp4r_gate.h")


def header_functions(path):
    return sorted(set(re.findall(r"^\s*(?:const\s+char\s*\*|int|void)\s+(icp4r_\w+)\s*\(", open(path).read(), re.M)))


def test_gate_abi():
    import icp4r

    L = icp4r.load()
    decl = header_functions(GATE_HEADER)
    for name in ("icp4r_compact_by_mask_batch_device", "icp4r_static_clouds_batch_device", "icp4r_static_cloud",
                 "icp4r_sequence_pairs", "icp4r_register_static_sequence"):
        assert name in decl
    assert sorted(icp4r.GATE_EXPORTED_SYMBOLS) == decl
    for name in decl:
        assert hasattr(L, name), f"{name} declared in icp4r_gate.h but not exported"
    assert L.icp4r_abi_version() == 6
    out = subprocess.run(["nm", "-D", "--defined-only", icp4r.library_path], capture_output=True, text=True).stdout
    for name in decl:
        assert re.search(rf"\bT {name}$", out, re.M), name
    # the ego header's own list is unchanged (tests/test_abi.py pins it)
    assert not set(decl) & set(icp4r.EGO_EXPORTED_SYMBOLS)


def _expand(counts, first, last):
    return [s for s in range(first, last + 1) for _ in range(counts[s])]


def _check_counts(counts):
    """The C entry's ranges == the literal loop's clouds, frame by frame; -> (registered frames,
    max non-empty scans in a registered target, in a registered source)."""
    from icp4r import ego

    counts = [int(c) for c in counts]
    sf, sl, tf, tl, reg = ego.sequence_pairs(counts)
    frames = gate_twin.sequence_pairs(counts)
    assert len(frames) == len(counts) == len(reg)
    max_t = max_s = 0
    for k, (registered, src, tgt) in enumerate(frames):
        assert bool(reg[k]) == registered, (counts, k)
        assert 0 <= sf[k] and sl[k] < len(counts) and 0 <= tf[k] and tl[k] < len(counts), (counts, k)
        assert _expand(counts, sf[k], sl[k]) == src, (counts, k)
        assert _expand(counts, tf[k], tl[k]) == tgt, (counts, k)
        if registered:
            max_t = max(max_t, sum(counts[s] > 0 for s in range(tf[k], tl[k] + 1)))
            max_s = max(max_s, sum(counts[s] > 0 for s in range(sf[k], sl[k] + 1)))
    assert max_t <= 1 and max_s <= 2, counts
    return int(np.sum(reg)), max_t, max_s


def test_sequence_pairs_exhaustive():
    """Every count vector of length <= 8 over {0, 3}."""
    cases, seen_t, seen_s = 0, 0, 0
    for n in range(0, 9):
        for counts in itertools.product((0, 3), repeat=n):
            _, t, s = _check_counts(counts)
            seen_t, seen_s = max(seen_t, t), max(seen_s, s)
            cases += 1
    assert cases == 2 ** 9 - 1
    assert (seen_t, seen_s) == (1, 2)  # both bounds are attained


def test_sequence_pairs_random():
    rng = np.random.default_rng(41)
    for _ in range(200):
        n = int(rng.integers(1, 41))
        counts = rng.integers(1, 50, n)
        counts[rng.random(n) < 0.3] = 0
        _check_counts(counts)


@pytest.mark.parametrize("empty", [[3], [0], [2, 3]])
def test_sequence_pairs_replay_cases(empty):
    """The three cases of tests/test_replay.py::test_replay_empty_scans_accumulate (6 frames)."""
    from icp4r import ego

    counts = [1024] * 6
    for k in empty:
        counts[k] = 0
    _check_counts(counts)
    sf, sl, tf, tl, reg = ego.sequence_pairs(counts)
    if empty == [0]:  # frames 0 and 1 skipped; frame 2: scans 1 + 2 against scan 1
        assert reg.tolist() == [0, 0, 1, 1, 1, 1]
        assert (sf[2], sl[2]) == (0, 2) and _expand(counts, tf[2], tl[2]) == [1] * 1024
    if empty == [3]:  # frame 3 skipped; frame 4: scan 4 against scan 2 (+ the empty scan 3)
        assert reg.tolist() == [1, 1, 1, 0, 1, 1]
        assert _expand(counts, sf[4], sl[4]) == [4] * 1024 and _expand(counts, tf[4], tl[4]) == [2] * 1024
    if empty == [2, 3]:  # frames 2 and 3 skipped; frame 4: scan 4 against scan 1, carried over
        assert reg.tolist() == [1, 1, 0, 0, 1, 1]
        assert _expand(counts, tf[4], tl[4]) == [1] * 1024


def test_sequence_pairs_refuses_negative_counts():
    import icp4r
    from icp4r import ego

    with pytest.raises(icp4r.ICP4RError):
        ego.sequence_pairs([3, -1, 3])


def test_twin_compact_layout():
    """The twin itself on a hand-made batch: order, the duplicated first entry, the oversized scan."""
    xyzi = np.arange(40, dtype=np.float32).reshape(10, 4)
    off, cnt = [6, 0, 3], [4, 3, 3]  # memory order != input order
    mask = np.array([1, 0, 1, 9, 9, 9, 0, 1, 1, 0], np.uint8)
    clouds, po, pn = gate_twin.compact(xyzi, off, cnt, mask, 3)
    assert pn.tolist() == [0, 0, 2, 3] and po.tolist() == [0, 0, 0, 2]  # scan 0 has cnt > max_n
    assert (clouds == xyzi[[0, 2, 3, 4, 5]]).all()
    clouds, po, pn = gate_twin.compact(xyzi, off, cnt, mask, 4, gate_twin.GATE_ALL)
    assert pn.tolist() == [4, 4, 3, 3] and po.tolist() == [0, 0, 4, 7]
    assert (clouds == xyzi[[6, 7, 8, 9, 0, 1, 2, 3, 4, 5]]).all()


def test_gate_host_check_under_sanitizers():
    """tests/cpp/gate_host_check: icp4r_sequence_pairs' host code against the literal loop over the
    exhaustive set, built with -fsanitize=address,undefined and run as a program."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "gate_host_check.mk"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "_build", "gate_host_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "511 cases, 0 mismatches" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
