"""GPU: every call of libsta_knn.so and the Python layer on it (cloud.NNIndex.knn, cloud.knn_moments) is ordered by its stream alone, also
behind pending work: the rows of tests/knn_stream_cases.py through the harness of tests/stream_cases.py (`references`, `delayed_call`)
on a side stream.  No row may return after the delay: knn_stream_cases.SYNCS is empty."""
import pytest

import knn_stream_cases as KS
import stream_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def side():
    """a frontend (for its pipeline streams: measured to overlap with the null stream) and one of those streams"""
    import torch
    from vista_slam_amd import weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)
    s = SC.side_streams(m, 1)[0]
    yield m, s
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", [r.name for r in KS.ROWS])
def test_a_call_behind_pending_work_equals_its_reference(side, name):
    m, s = side
    row = KS.by_name(name)
    assert not KS.may_wait(row)
    xa, xb, ref_a, ref_b = SC.references(row, m, s)
    rep = SC.delayed_call(row, m, s, xa, xb, ref_a, ref_b)
    print(f"[knn stream] {name} ({row.shapes}): {rep.line()}")
    if rep.waited:
        pytest.fail(f"{name}: the call returned after the delay of {rep.delay_ms:.1f} ms had ended (host time on an idle stream {rep.host_ms:.2f} ms): "
                    "an entry documented as asynchronous waited for its stream, or the delay was too short")
    assert rep.diff is None, f"{name}: behind pending work on its stream the call differs from its reference - {rep.diff}"
