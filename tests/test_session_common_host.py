"""CPU checks of ``spiking_fullsubnet_amd/session_common.py``: ``row_count_jobs`` against the three builders it replaced (restated
here field by field), and what the mixin may and may not be -- listed by both session classes, state-less, and without any of the
names a session must not acquire (tests/test_cirm_hold_host.py's ``PINNED``).  No device, no library call."""
import inspect

import pytest
import torch

from test_cirm_hold_host import PINNED


def old_builder(tens, counts, T=None, R=None):
    """What ``StreamingSession.__init__``, ``FullbandStreamingSession._build_sequence`` (T = R = None: the tensors' own sizes) and
    ``FullbandStreamingSession._catch_up_run`` (T, R given) wrote, as plain tuples."""
    from spiking_fullsubnet_amd._lib import MAX_COUNT_TENSORS
    out = []
    for i0 in range(0, len(tens), MAX_COUNT_TENSORS):
        out.append([(t.data_ptr(), t.shape[0] if T is None else T, t.shape[1] if R is None else R, t.shape[2], rpc, counts[i0 + j].data_ptr())
                    for j, (t, rpc) in enumerate(tens[i0:i0 + MAX_COUNT_TENSORS])])
    return out


@pytest.mark.parametrize("n", [1, 16, 17])
@pytest.mark.parametrize("given", [False, True])
def test_row_count_jobs_fills_what_the_three_builders_filled(n, given):
    from spiking_fullsubnet_amd._lib import MAX_COUNT_TENSORS, RowCount
    from spiking_fullsubnet_amd.session_common import row_count_jobs
    assert MAX_COUNT_TENSORS == 16
    # tensors of different sizes and rows per clip, so that no field can stand in for another
    tens = [(torch.zeros((5 + i, 3 * (1 + i % 4), 64 * (1 + i % 2)), dtype=torch.int8), 1 + i % 4) for i in range(n)]
    counts = torch.zeros((n, 3), dtype=torch.int64)
    T, R = (4, 2) if given else (None, None)
    jobs = row_count_jobs(tens, counts, T=T, R=R)
    want = old_builder(tens, counts, T, R)
    assert [len(a) for a in jobs] == [len(w) for w in want] == ([n] if n <= 16 else [16, n - 16])
    for arr, rows in zip(jobs, want):
        assert isinstance(arr, RowCount * len(rows))
        got = [(a.spikes_i8, a.T, a.R, a.HP, a.rows_per_clip, a.counts) for a in arr]
        assert got == rows
    # every job has its own spikes and its own row of counts, 8 bytes x 3 clips apart
    flat = [a for arr in jobs for a in arr]
    assert len({a.spikes_i8 for a in flat}) == n and [a.counts - flat[0].counts for a in flat] == [24 * i for i in range(n)]
    if not given:
        assert [(a.T, a.R, a.HP) for a in flat] == [tuple(t.shape) for t, _ in tens]
    else:
        assert {(a.T, a.R) for a in flat} == {(4, 2)}


def test_both_sessions_list_the_mixin_and_it_is_stateless():
    from spiking_fullsubnet_amd import session_common
    from spiking_fullsubnet_amd.fullband_streaming import FullbandStreamingSession
    from spiking_fullsubnet_amd.streaming import StreamingSession
    mixin = session_common.SessionCommon
    for cls in (StreamingSession, FullbandStreamingSession):
        assert cls.__bases__ == (mixin,)  # the mixin and nothing else: neither session inherits from the other
    assert mixin.__bases__ == (object,)
    assert "__init__" not in mixin.__dict__ and "__getattr__" not in mixin.__dict__ and "__slots__" not in mixin.__dict__
    for name in PINNED:
        assert name not in mixin.__dict__ and not hasattr(mixin, name)
    # nothing public, no property (clip_frames / clip_calls stay each class's own), and no data but the one static function
    for name, v in mixin.__dict__.items():
        if name.startswith("__"):
            continue
        assert name.startswith("_"), name
        assert not isinstance(v, property), name
        assert inspect.isfunction(v) or isinstance(v, staticmethod), name
    assert isinstance(StreamingSession.__dict__["clip_frames"], property) and isinstance(StreamingSession.__dict__["clip_calls"], property)
    assert inspect.isfunction(FullbandStreamingSession.__dict__["clip_frames"]) and inspect.isfunction(FullbandStreamingSession.__dict__["clip_calls"])
    # what the mixin holds is defined once: neither class overrides it
    shared = [n for n in mixin.__dict__ if not n.startswith("__")]
    assert "_as_i32" in shared and "_held_bookkeeping" in shared and "_state_layout" in shared and "_capture" in shared
    for cls in (StreamingSession, FullbandStreamingSession):
        assert not [n for n in shared if n in cls.__dict__], cls
        assert cls._as_i32(0xFFFFFFFF) == -1 and cls._as_i32(1 << 32) == 0


def test_the_cirm_session_keeps_its_step_signatures_and_has_three_bodies():
    from spiking_fullsubnet_amd.fullband_streaming import FullbandStreamingSession as cls
    assert list(inspect.signature(cls.step).parameters) == ["self", "frames", "copy"]
    assert list(inspect.signature(cls.step_wave).parameters) == ["self", "samples", "copy"]
    assert list(inspect.signature(cls.step_wave_host).parameters) == ["self", "samples", "timeout_s"]
    assert inspect.signature(cls.step).parameters["copy"].default is True and inspect.signature(cls.step_wave).parameters["copy"].default is True
    assert inspect.signature(cls.step_wave_host).parameters["timeout_s"].default == 2.0
    assert list(inspect.signature(cls._call).parameters) == ["self", "frames", "hold", "copy"]
    assert list(inspect.signature(cls._call_wave).parameters) == ["self", "samples", "hold", "copy"]
    assert list(inspect.signature(cls._call_wave_host).parameters) == ["self", "samples", "hold", "timeout_s"]
    for name in PINNED:
        assert not hasattr(cls, name)
