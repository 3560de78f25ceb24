"""The reference's own ikd-Tree behind oracle/ref/ikd_ref_driver.cpp — TEST INFRASTRUCTURE ONLY.

`make -C oracle ref` builds oracle/_ref/ikd_ref from the reference project's ikd_Tree.{h,cpp}; this module
writes the driver's job file, runs it and parses what the tree answered.  It opens no GPU and the product
path never imports it.

    job = Job(0.3, 0.6, 0.5)
    job.build(frame0); job.set_downsample(0.5)
    job.add(frame1); job.sector(centre, 80.0, heading); job.size()
    results = job.run()          # one entry per call, in order

build/add take (n, >=3) float32 points; a point's index (its position over all builds and adds of the job,
unless `first` says otherwise) travels in the intensity, and every search returns sorted int32 indices.
"""
from __future__ import annotations

import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")  # oracle/Makefile's variable and default
REF_DIR = os.path.join(HERE, "_ref")
EXE = os.path.join(REF_DIR, "ikd_ref")
BINARIES = ("ikd_ref", "ref_map_callsite", "ref_map_edit_callsite")
MAGIC = 0x4A444B49

BUILD, ADD, SET_DOWNSAMPLE, SECTOR, BOX, RADIUS, DELETE_BOXES, SIZE, HEADING_TABLE = range(1, 10)


def available() -> bool:
    """True where the driver binary is present and executable."""
    return os.path.isfile(EXE) and os.access(EXE, os.X_OK)


def _xyz(points) -> np.ndarray:
    p = np.asarray(points, np.float32)
    return np.ascontiguousarray(p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)[:, :3], "<f4")


class Job:
    def __init__(self, delete_param: float = 0.5, balance_param: float = 0.6, box_length: float = 0.2):
        self._buf = [struct.pack("<I3f", MAGIC, delete_param, balance_param, box_length)]
        self._ops = []
        self._next = 0

    def _points(self, points, first):
        xyz = _xyz(points)
        first = self._next if first is None else int(first)
        self._next = max(self._next, first + len(xyz))
        return xyz, first

    def build(self, points, first=None):
        xyz, first = self._points(points, first)
        self._ops.append(BUILD)
        self._buf += [struct.pack("<IIi", BUILD, len(xyz), first), xyz.tobytes()]

    def add(self, points, downsample_on: bool = False, first=None):
        xyz, first = self._points(points, first)
        self._ops.append(ADD)
        self._buf += [struct.pack("<IIiI", ADD, len(xyz), first, int(bool(downsample_on))), xyz.tobytes()]

    def set_downsample(self, box_length: float):
        self._ops.append(SET_DOWNSAMPLE)
        self._buf.append(struct.pack("<If", SET_DOWNSAMPLE, box_length))

    def sector(self, center, radius: float, heading: float):
        self._ops.append(SECTOR)
        self._buf.append(struct.pack("<I5f", SECTOR, *_xyz(center)[0].tolist(), radius, heading))

    def box(self, box):
        self._ops.append(BOX)
        self._buf.append(struct.pack("<I", BOX) + np.asarray(box, "<f4").reshape(6).tobytes())

    def radius(self, center, radius: float):
        self._ops.append(RADIUS)
        self._buf.append(struct.pack("<I4f", RADIUS, *_xyz(center)[0].tolist(), radius))

    def delete_boxes(self, boxes):
        b = np.ascontiguousarray(np.asarray(boxes, "<f4").reshape(-1, 6))
        self._ops.append(DELETE_BOXES)
        self._buf += [struct.pack("<II", DELETE_BOXES, len(b)), b.tobytes()]

    def size(self):
        self._ops.append(SIZE)
        self._buf.append(struct.pack("<I", SIZE))

    def heading_table(self, points, centers):
        pairs = np.ascontiguousarray(np.concatenate([_xyz(points), _xyz(centers)], axis=1), "<f4")
        self._ops.append(HEADING_TABLE)
        self._buf += [struct.pack("<II", HEADING_TABLE, len(pairs)), pairs.tobytes()]

    def run(self) -> list:
        """Runs the job on the real tree.  Per op: build / set_downsample -> None; add -> counter;
        delete_boxes -> deleted; sector / box / radius -> sorted int32 indices; size -> (size, validnum, rebuilds
        handed to the rebuild thread so far: timing-dependent, zero or not is what it tells);
        heading_table -> (calc_heading bits, calc_dist bits) as uint32 arrays."""
        if not available():
            raise RuntimeError(f"{EXE} is not built (make -C oracle ref)")
        with tempfile.TemporaryDirectory(prefix="ikd_ref_") as tmp:
            job, res = os.path.join(tmp, "job.bin"), os.path.join(tmp, "result.bin")
            with open(job, "wb") as f:
                f.write(b"".join(self._buf))
            r = subprocess.run([EXE, job, res], capture_output=True, text=True, timeout=60)
            if r.returncode != 0:
                raise RuntimeError(f"ikd_ref failed ({r.returncode}): {r.stderr.strip()}")
            with open(res, "rb") as f:
                raw = f.read()
        out, pos = [], 0
        for op in self._ops:
            got, nwords = struct.unpack_from("<II", raw, pos)
            if got != op:
                raise RuntimeError(f"ikd_ref answered op {got} where {op} was asked")
            words = np.frombuffer(raw, "<u4", nwords, pos + 8)
            pos += 8 + 4 * nwords
            if op in (BUILD, SET_DOWNSAMPLE):
                out.append(None)
            elif op in (ADD, DELETE_BOXES):
                out.append(int(words.view("<i4")[0]))
            elif op == SIZE:
                out.append(tuple(int(v) for v in words.view("<i4")[:3]))
            elif op == HEADING_TABLE:
                out.append((words[: nwords // 2].astype(np.uint32), words[nwords // 2:].astype(np.uint32)))
            else:
                out.append(words.view("<i4").astype(np.int32))
        if pos != len(raw):
            raise RuntimeError("ikd_ref wrote more than was asked")
        return out
