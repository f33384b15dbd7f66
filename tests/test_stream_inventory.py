"""Host only: every entry point of include/sta_mi355.h that takes a stream has a row in tests/stream_cases.py (the matrix of
tests/test_stream_order_gpu.py) or a reason in its EXEMPT, and every entry point a row names exists - so an entry point added later
without a row fails here, without a GPU (tests/test_workspace_inventory.py does the same for the scratch contexts).

The parser: a declaration starts at `STA_API` and ends at the next `;`; it takes a stream when its last parameter is `void* stream`."""
import pathlib
import re

import stream_cases as SC
import workspace_cases as WC
from vista_slam_amd import _lib

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "sta_mi355.h"
DECL = re.compile(r"\bSTA_API\b([^;{]*?)\b([A-Za-z_]\w*)\s*\(([^;]*)\)\s*;", re.S)


def stream_entry_points(text):
    """-> (all declared entry points, those whose last parameter is `void* stream`)"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    every, taking = [], []
    for m in DECL.finditer(text):
        name, params = m.group(2), [p.strip() for p in m.group(3).split(",")]
        every.append(name)
        if re.fullmatch(r"void\s*\*\s*stream", params[-1]):
            taking.append(name)
    return every, taking


def test_parser_sees_the_known_shapes_of_a_declaration():
    text = ("STA_API int sta_one(sta_handle* h, void* stream);\n"
            "STA_API int sta_two(sta_handle* h, const float* x, /* a comment, with (brackets); */\n"
            "                    int n, void *stream);\n"
            "STA_API int sta_streams(sta_handle* h, void* const* streams, int n_streams);\n"
            "STA_API const char* sta_text(void);\n"
            "STA_API int sta_mid(sta_handle* h, void* stream, int flag);   // void* stream);\n"
            "int not_exported(void* stream);\n")
    every, taking = stream_entry_points(text)
    assert every == ["sta_one", "sta_two", "sta_streams", "sta_text", "sta_mid"] and taking == ["sta_one", "sta_two"]


def test_every_stream_entry_point_has_a_row():
    every, taking = stream_entry_points(HEADER.read_text())
    assert len(taking) >= 50 and len(set(taking)) == len(taking), len(taking)          # (else the parser itself went blind)
    assert set(every) == set(_lib.SIGNATURES), sorted(set(every) ^ set(_lib.SIGNATURES))
    named = SC.named_entries()
    assert not (named & set(SC.EXEMPT)), sorted(named & set(SC.EXEMPT))
    missing = sorted(set(taking) - named - set(SC.EXEMPT))
    assert not missing, f"entry points that take a stream without a row in tests/stream_cases.py (or a reason in its EXEMPT): {missing}"
    unknown = sorted(named - set(_lib.SIGNATURES))
    assert not unknown, f"tests/stream_cases.py names entry points the ABI does not have: {unknown}"
    no_stream = sorted((named | set(SC.EXEMPT)) - set(taking))
    assert not no_stream, f"tests/stream_cases.py names entry points that take no stream: {no_stream}"
    for name, reason in SC.EXEMPT.items():
        assert reason.strip(), name


def test_the_matrix_is_well_formed():
    names = [r.name for r in SC.ROWS]
    assert len(names) == len(set(names))
    for r in SC.ROWS:
        assert r.entries and r.shapes and callable(r.make) and callable(r.run), r.name
        assert r.make_b is None or callable(r.make_b), r.name
        assert set(r.no_prec) <= set(WC.PRECISIONS), r.name
    assert [r.name for r in SC.ROWS[:len(WC.CASES)]] == [c.name for c in WC.CASES]     # the workspace rows, unchanged and all of them
    assert all(r.make is c.make and r.run is c.run and r.entries == c.entries for r, c in zip(SC.ROWS, WC.CASES))
    assert set(SC.PRECISIONS) <= set(WC.PRECISIONS) and SC.runs()
    keys = SC.named_entries() | SC.named_layers()
    assert set(SC.SYNCS) <= keys, sorted(set(SC.SYNCS) - keys)
    for name, sentence in SC.SYNCS.items():
        assert sentence.strip(), name
    assert SC.DELAY_FACTOR == 4.0 and SC.MAX_STREAMS <= 12
