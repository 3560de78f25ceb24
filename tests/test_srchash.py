"""tools/srchash.py covers every ICP kernel unit the Makefile builds and every csrc header (no GPU)."""
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import srchash  # noqa: E402

CSRC = os.path.join(ROOT, "icp-4dradar_amd", "csrc")


def test_units_exist_and_are_hashed():
    units = srchash.icp_units()
    assert units, "the Makefile's ICP_UNITS line names no unit"
    hashed = set(srchash.icp_source_files())
    for u in units:
        path = os.path.join(CSRC, u + ".hip")
        assert os.path.isfile(path), path
        assert path in hashed, path


def test_every_csrc_header_is_hashed():
    headers = glob.glob(os.path.join(CSRC, "*.hpp"))
    assert headers
    assert set(headers) <= set(srchash.icp_source_files())


def test_hash_is_computed():
    assert srchash.icp_sources_sha256() is not None
