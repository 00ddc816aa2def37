"""Host side of the per-sequence sampling controls: generate.sampling_rows broadcasts and validates the controls (the
kernels do not), and the JSON form of the log-probabilities that generate.py --logprobs writes."""
import numpy as np
import pytest


def test_sampling_rows_broadcasts_numbers_and_sequences():
    from commu_amd.generate import sampling_rows
    t, k, p = sampling_rows(4, 0.95, 32, 1.0)
    assert t.dtype == np.float32 and k.dtype == np.int32 and p.dtype == np.float32
    assert t.tolist() == [np.float32(0.95)] * 4 and k.tolist() == [32] * 4 and p.tolist() == [1.0] * 4
    t, k, p = sampling_rows(3, [0.0, 0.95, 1.3], 8, (0.5, 1.0, 0.9))
    assert t.tolist() == [0.0, np.float32(0.95), np.float32(1.3)] and k.tolist() == [8, 8, 8]
    assert p.tolist() == [0.5, 1.0, np.float32(0.9)]
    t, k, p = sampling_rows(2, np.array([0.5, 2.0]), np.array([1, 729]), 1)
    assert t.tolist() == [0.5, 2.0] and k.tolist() == [1, 729] and p.tolist() == [1.0, 1.0]
    assert sampling_rows(1, 0, 1)[2].tolist() == [1.0]                # top_p defaults to "off"
    assert [a.shape for a in sampling_rows(0, [], [], [])] == [(0,)] * 3


@pytest.mark.parametrize("bad", [
    dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")),
    dict(temperature=[0.95, -1.0, 0.95]),
    dict(top_k=0), dict(top_k=730), dict(top_k=-3), dict(top_k=[32, 0, 32]), dict(top_k=2.5), dict(top_k=float("nan")),
    dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=float("nan")), dict(top_p=1.01), dict(top_p=[1.0, 0.5, 0.0]),
    dict(temperature=[0.95, 0.95]), dict(top_k=[32] * 4), dict(top_p=[[1.0, 1.0, 1.0]]), dict(temperature="hot"),
    dict(top_k=None),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_sampling_rows_refuses(bad):
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import sampling_rows
    args = dict(temperature=0.95, top_k=32, top_p=1.0)
    args.update(bad)
    with pytest.raises(CommuHipError):
        sampling_rows(3, **args)


def test_logprobs_json_form():
    from commu_amd.midi_generator.replicas import logprobs_to_lists
    nan = float("nan")
    lp = np.array([[nan, nan], [-1.5, -0.25], [nan, nan], [-3.0, 0.0]], dtype=np.float32)
    assert logprobs_to_lists([lp, None]) == [[None, [-1.5, -0.25], None, [-3.0, 0.0]], None]
