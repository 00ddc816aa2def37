"""Primed generation, host side (no GPU): the plain-Python replay contract (tests/prime_contract.py) pinned to the
reference's own fixtures (tests/golden/g6_decode.npz), the planted divergences, and the CLI option."""
import os

import numpy as np
import pytest

import prime_contract as P


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "g6_decode.npz"))


# fed-stream entries of the full sequence (without its EOS); with the EOS offered as well the replay makes one more step
# before it reports the EOS
ENTRIES = {"greedy8": 260, "greedy5": 200, "sample8": 68, "sample8m": 102}


@pytest.mark.parametrize("tag", sorted(ENTRIES))
def test_fed_stream_of_the_full_sequence_is_the_reference_trace(z, tag):
    """The fed stream of the fixture's whole sequence equals the token column of the reference's trace entry for entry,
    the memory lengths follow from the keep flags (first step discarded, forced tokens doubled), and at every cut point
    a prefix of the prompt yields a prefix of the stream and of the sequence."""
    ctx, ct, cp, nm, p = P.fixture(z, tag)
    trace = z[f"{tag}_trace"]
    s, seq, fed, div = P.replay(ctx, ct, cp, nm, p)
    assert div == (-1, -1)
    assert len(fed) == ENTRIES[tag] <= len(trace)
    assert [t for t, _ in fed] == trace[:len(fed), 0].tolist()
    klen = len(ctx) - 1
    for i, (_, k) in enumerate(fed):
        assert trace[i, 1] == klen and trace[i, 2] == klen + 1
        klen += k
    assert fed[0][1] == 0 and all(k == 1 for _, k in fed[1:])
    assert seq == ctx + p and s[P.F_LEN] == len(seq)
    assert s[P.F_ITERS] == 0 and s[P.F_NDRAW] == 0 and s[P.F_NTRACE] == len(fed) and s[P.F_FORCED] == -1
    assert s[P.F_NBAR] == p.count(P.BAR)
    for k in range(len(p) + 1):
        s_k, seq_k, fed_k, div_k = P.replay(ctx, ct, cp, nm, p[:k])
        assert div_k == (-1, -1) and seq_k == ctx + p[:k]
        assert fed_k == fed[:len(fed_k)], k
        assert s_k[P.F_FORCED] == -1 and s_k[P.F_NTRACE] == len(fed_k)
    full = [int(t) for t in z[f"{tag}_seq"]][len(ctx):]
    if full[-1] == P.EOS:          # offered too, the EOS is reported where it stands, one model step later
        _, _, fed_e, div_e = P.replay(ctx, ct, cp, nm, full)
        assert div_e[0] == len(full) - 1 and len(fed_e) == len(fed) + 1
        assert [t for t, _ in fed_e] == trace[:len(fed_e), 0].tolist()


def test_end_records_of_the_fixture_replays(z):
    want = {"greedy8": (3, 3), "greedy5": (4, 3), "sample8": (8, 8), "sample8m": (8, 8)}
    for tag, (nbar, cur) in want.items():
        ctx, ct, cp, nm, p = P.fixture(z, tag)
        s = P.replay(ctx, ct, cp, nm, p)[0]
        assert (s[P.F_NBAR], s[P.F_CUR]) == (nbar, cur), tag


def test_empty_prompt_returns_the_initial_record(z):
    ctx, ct, cp, nm, _ = P.fixture(z, "greedy8")
    s, seq, fed, div = P.replay(ctx, ct, cp, nm, [])
    assert s == P.initial_record(len(ctx) - 1, len(ct), nm) and seq == ctx and fed == [] and div == (-1, -1)
    assert s[P.F_FIRST] == 1


def test_mid_bar_chord_position_is_fed_once_by_the_replay(z):
    """The documented limitation: where the loop replaced a draw by a forced mid-bar chord position (sample4x, chord
    positions 496, length_fit false) the real run fed that position twice; the replay feeds it once.  No divergence, the
    same tokens and end state; the trace differs first at entry 7."""
    ctx, ct, cp, nm, p = P.fixture(z, "sample4x")
    s, seq, fed, div = P.replay(ctx, ct, cp, nm, p)
    assert div == (-1, -1) and seq == ctx + p
    assert (s[P.F_CUR], s[P.F_NBAR], s[P.F_LENGTH_FIT]) == (6, 4, 0)
    trace = z["sample4x_trace"][:, 0].tolist()
    col = [t for t, _ in fed]
    first = next(i for i in range(min(len(col), len(trace))) if col[i] != trace[i])
    assert first == 7
    assert trace[6] == trace[7] == 496 and col[6] == 496          # fed twice by the loop, once by the replay


def test_planted_divergences_are_reported_at_their_index(z):
    cases = P.planted(z)
    assert len(cases) == 6
    for name, tag, prompt, want in cases:
        ctx, ct, cp, nm, _ = P.fixture(z, tag)
        div = P.replay(ctx, ct, cp, nm, prompt)[3]
        assert div == want, name
        # the prefix before the index is fine
        assert P.replay(ctx, ct, cp, nm, prompt[:want[0]])[3] == (-1, -1), name
    ctx, ct, cp, nm, _ = P.fixture(z, "greedy8")
    assert P.replay(ctx, ct, cp, nm, [500, 729])[3] == (1, P.INVALID)


def test_cut_points_cover_the_named_places(z):
    for tag in P.TAGS:
        p = P.fixture(z, tag)[4]
        cuts = P.cut_points(p)
        assert cuts[0] == 0 and cuts[1] == 1 and cuts[-1] == len(p)
        assert any(k >= 1 and p[k - 1] == P.BAR for k in cuts)
        assert any(k >= 2 and p[k - 2] == P.BAR and p[k - 1] == P.POS0 for k in cuts)
        assert any(k >= 1 and P.CHORD_LO <= p[k - 1] <= P.CHORD_HI for k in cuts)


def test_cli_parser_accepts_prompt_tokens(tmp_path):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("commu_generate_cli", os.path.join(root, "commu-code_amd", "generate.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    f = tmp_path / "prompt.json"
    f.write_text("[2, 432, 199, 500]")
    assert cli.read_prompt_tokens(str(f)) == [2, 432, 199, 500]
    args, _ = cli.parse_args()["input_args"].parse_known_args(["--output_dir", str(tmp_path), "--prompt_tokens", str(f)])
    assert args.prompt_tokens == str(f)
    args, _ = cli.parse_args()["input_args"].parse_known_args(["--output_dir", str(tmp_path)])
    assert args.prompt_tokens is None
    f.write_text('{"tokens": [1]}')
    with pytest.raises(ValueError):
        cli.read_prompt_tokens(str(f))
