"""The map-maintenance entries of include/icp4r/icp4r_map.h are declared, listed and exported, and the
ABI version did not move (they are additions).  No GPU calls."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_HEADER = os.path.join(ROOT, "include", "icp4r", "icp4r_map.h")

OLD = ["icp4r_map_create", "icp4r_map_destroy", "icp4r_map_build", "icp4r_map_add_points", "icp4r_map_add_scan",
       "icp4r_map_size", "icp4r_map_sector_search", "icp4r_map_sector_search_device", "icp4r_map_points_device",
       "icp4r_map_time_ms", "icp4r_map_time_reset"]
NEW = ["icp4r_map_delete_boxes", "icp4r_map_box_search", "icp4r_map_radius_search", "icp4r_map_box_search_device",
       "icp4r_map_radius_search_device", "icp4r_map_add_points_downsample"]


def test_header_declares_the_edit_entries():
    import icp4r

    decl = re.findall(r"^\s*int\s+(icp4r_\w+)\s*\(", open(MAP_HEADER).read(), re.M)
    assert sorted(decl) == sorted(OLD + NEW)
    assert sorted(icp4r.MAP_EXPORTED_SYMBOLS) == sorted(OLD + NEW)


def test_library_exports_the_edit_entries():
    import icp4r

    L = icp4r.load()
    out = subprocess.run(["nm", "-D", "--defined-only", icp4r.library_path], capture_output=True, text=True).stdout
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(rf"\bT {name}$", out, re.M), name
        assert getattr(L, name).argtypes is not None, name  # prototyped for ctypes
    assert L.icp4r_abi_version() == 6


def test_detached_wording_is_documented():
    """The header states the lifetime rule the library enforces."""
    text = " ".join(open(MAP_HEADER).read().split())
    assert "may outlive its context" in text and "Destroy it before its context" not in text
