"""Host only: libsta_cloud.so exports exactly include/sta_cloud.h, the ctypes table mirrors it, every declaration that takes a stream
has a row in tests/cloud_stream_cases.py (and the other way round), and the product library's export table did not move."""
import os
import pathlib

import cloud_stream_cases as CS
from test_cabi_symbols import all_exported, declared_symbols, exported_symbols
from test_stream_inventory import stream_entry_points

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "sta_cloud.h"
LINKER = {"_init", "_fini", "_edata", "_end", "__bss_start"}


def test_the_library_exports_exactly_its_header():
    from vista_slam_amd import _lib, build
    build.build_lib()
    every, _taking = stream_entry_points(HEADER.read_text())
    assert len(every) == len(set(every)) == 5, every
    assert set(every) == set(_lib.CLOUD_SIGNATURES), set(every) ^ set(_lib.CLOUD_SIGNATURES)
    assert all_exported(_lib.CLOUD_LIB_PATH) - LINKER == set(every), sorted(all_exported(_lib.CLOUD_LIB_PATH) - LINKER ^ set(every))
    assert not (set(every) & set(_lib.SIGNATURES)) and not (set(every) & set(_lib.TEST_SIGNATURES))
    lib = _lib.load_cloud()
    for name in every:
        assert hasattr(lib, name), name


def test_every_stream_entry_point_has_a_row():
    _every, taking = stream_entry_points(HEADER.read_text())
    assert sorted(taking) == ["sta_cloud_transform", "sta_nn_build", "sta_nn_query"], taking
    named = CS.named_entries()
    assert not (named & set(CS.EXEMPT))
    assert not set(taking) - named - set(CS.EXEMPT), sorted(set(taking) - named - set(CS.EXEMPT))
    assert not (named | set(CS.EXEMPT)) - set(taking), sorted((named | set(CS.EXEMPT)) - set(taking))
    names = [r.name for r in CS.ROWS]
    assert len(names) == len(set(names))
    for r in CS.ROWS:
        assert r.entries and r.shapes and callable(r.make) and callable(r.run) and callable(r.make_b), r.name
    assert set(CS.SYNCS) <= named | CS.named_layers()
    header = HEADER.read_text()
    assert "SYNCHRONISES `stream` once" in header            # the sentence SYNCS quotes
    for name, sentence in CS.SYNCS.items():
        assert sentence.strip(), name


def test_the_product_library_is_what_it_was():
    """The cloud entry points are a library of their own: the product's export table is include/sta_mi355.h, none of the new names
    is in it, and nothing of the new translation unit is among the sources the product's hash covers."""
    from vista_slam_amd import _lib, build
    prod = declared_symbols("sta_mi355.h")
    assert exported_symbols(_lib.LIB_PATH) == prod == set(_lib.SIGNATURES)
    assert all_exported(_lib.LIB_PATH) - LINKER == prod
    assert not {s for s in all_exported(_lib.LIB_PATH) if "cloud_" in s or s.startswith("sta_nn_")} - {"sta_world_pointcloud"}
    assert len(prod) >= 48
    assert not {"sta_cloud.hip", "cloud.h", os.path.join("..", "..", "include", "sta_cloud.h")} & set(build.DEPS)
    assert {"sta_cloud.hip", "cloud.h", "voxel.h"} <= set(build.CLOUD_DEPS)
    assert build.source_hash() != build.source_hash(build.CLOUD_DEPS)
    assert not build.is_stale(build.CLOUD_LIB, build.CLOUD_HASH_FILE, build.CLOUD_DEPS)
