"""CPU-side checks of the sliding decode memory (the ring K/V cache of csrc/decode.hip and csrc/parity_f32.hip):
the command line and the configuration plumbing, and the ring index arithmetic the kernels implement, restated here in
plain Python and checked against a list that slides the way the reference's memory does (commu/model/model.py:507-568)."""
import importlib.util
import os
import random
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    spec = importlib.util.spec_from_file_location("commu_cli_generate_sliding",
                                                  os.path.join(ROOT, "commu-code_amd", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags_and_their_defaults():
    """--memory_length / --generation_length / --sliding_memory: parsed as model arguments; without them the inference
    configuration keeps the reference's 4146 / 4096 and the memory does not slide; with them the configuration the
    generator reads carries the values (and no key is added to the configuration unless the switch is given)."""
    from commu_amd.midi_generator.model_initializer import ModelInitializeTask
    parser = _cli().parse_args()["model_args"]
    margs, _ = parser.parse_known_args(["--checkpoint_dir", "x.pt", "--output_dir", "o"])
    assert margs.sliding_memory is False and margs.memory_length is None and margs.generation_length is None
    cfg = ModelInitializeTask(margs).inference_cfg
    assert cfg.MODEL.memory_length == 4146 and cfg.GENERATION.generation_length == 4096
    assert "sliding_memory" not in cfg.GENERATION and getattr(cfg.GENERATION, "sliding_memory", False) is False
    margs, _ = parser.parse_known_args(["--checkpoint_dir", "x.pt", "--memory_length", "512", "--generation_length", "2048",
                                        "--sliding_memory", "--output_dir", "o"])
    assert (margs.memory_length, margs.generation_length, margs.sliding_memory) == (512, 2048, True)
    cfg = ModelInitializeTask(margs).inference_cfg
    assert cfg.MODEL.memory_length == 512 and cfg.GENERATION.generation_length == 2048
    assert cfg.GENERATION.sliding_memory is True
    # callers that hand over a bare namespace (no new attributes) get the reference's configuration
    cfg = ModelInitializeTask(types.SimpleNamespace(checkpoint_dir="x.pt")).inference_cfg
    assert cfg.MODEL.memory_length == 4146 and "sliding_memory" not in cfg.GENERATION


def test_reference_schema_has_no_sliding_key():
    from commu_amd.model.config_helper import get_default_cfg_inference
    assert "sliding_memory" not in get_default_cfg_inference().GENERATION


# ---- the ring arithmetic of the kernels (W = M + 1 rows; klen counts absolute positions) ----------------------------
def ring_view(pos, M, same_length):
    """What the bf16 ring kernel derives from klen[b] = pos: (row the new token is written to, number of physical rows
    0 .. nvalid - 1 it streams, distance of every streamed row, the hidden row or -1)."""
    W = M + 1
    cur = pos % W
    nvalid = min(pos + 1, W)
    dist = []
    for j in range(nvalid):
        d = cur - j
        if d < 0:
            d += W
        dist.append(d)
    masked = -1
    if same_length and pos >= W - 1:
        masked = 0 if cur + 1 == W else cur + 1
    return cur, nvalid, dist, masked


def ring_view_f32(pos, M, same_length):
    """The fp32 kernel walks positions lo .. pos in chronological order: [(row, distance)]."""
    W = M + 1
    lo = pos - M if pos > M else 0
    if same_length and pos >= M:
        lo += 1
    wrap = (pos // W) * W
    return [((p - wrap) if p >= wrap else (p - wrap + W), pos - p) for p in range(lo, pos + 1)]


def test_ring_index_arithmetic_against_a_sliding_list():
    """A few thousand random (M, same_length) runs with kept and discarded steps (quirk Q3): the memory is a Python list
    that keeps the last M positions (model.py:524-536); the new token sees the memory plus itself, minus the oldest key
    when same_length is on and the memory is full (model.py:551-568 with qlen 1).  The ring must expose exactly those
    positions at exactly those distances, and a discarded step must leave every live row as it was."""
    rnd = random.Random(7)
    checked = 0
    for _ in range(400):
        M = rnd.choice([1, 2, 3, 5, 16, 31, 32, 48, 96])
        same_length = rnd.random() < 0.5
        W = M + 1
        ring = [None] * W                      # row -> absolute position stored there
        mem = []                               # the reference's memory: absolute positions, oldest first
        pos = 0
        for _ in range(rnd.randint(1, 6 * W)):
            keep = rnd.random() < 0.85
            cur, nvalid, dist, masked = ring_view(pos, M, same_length)
            before = list(ring)
            ring[cur] = pos                    # the fused K/V append
            # reference: keys = memory + the new token; same_length hides the oldest once the memory is full
            keys = mem + [pos]
            if same_length and len(mem) >= M:
                keys = keys[1:]
            want = {p: pos - p for p in keys}
            got = {ring[j]: dist[j] for j in range(nvalid) if j != masked}
            assert got == want, (M, same_length, pos)
            assert all(0 <= d <= M for d in dist)
            assert len(want) == (M if same_length and pos >= M else min(pos, M) + 1)
            # the row that was overwritten held nothing the memory still needs
            assert before[cur] is None or before[cur] not in mem
            # fp32 kernel: same set, chronological order
            f32 = ring_view_f32(pos, M, same_length)
            assert [ring[r] for r, _ in f32] == sorted(want) and all(want[ring[r]] == d for r, d in f32)
            if keep:
                mem = (mem + [pos])[-M:]
                pos += 1
            checked += 1
    assert checked > 5000
