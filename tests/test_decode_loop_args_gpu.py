"""The two host paths into the sampling stage of the decode loop fill two different argument structs (commu_sample_args
through ForcedDecoder.iteration(), commu_decode_loop_args through body_pre()): for every kernel selector they must decode
the same tokens and leave the same records.  A field filled wrongly in one path and not in the other shows here (tried
with a null gram_on and with a null harm_on in body_pre only: the grammar selectors, resp. the harmony selector, fail)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_decode_gpu as TD  # noqa: E402

B, GLEN, ITERS = 3, 6, 6          # ld_seq = 16 + GLEN + 2 = 24
SELECTORS = ["none", "bias", "grammar", "grammar_bias", "harmony"]


@pytest.fixture(scope="module")
def fixture_model(golden_dir):
    z = TD.load(golden_dir, "g6_decode.npz")
    return z, TD._build(golden_dir, z, z["sample8m_bias"])


def decoder(z, model, selector):
    from commu_amd.generate import ForcedDecoder, token_constraints
    dec = ForcedDecoder(model, B, GLEN, 4146, 0.95, 32)
    assert dec.ld_seq == 24 and dec.wrong.shape[1] == 729
    if "bias" in selector:
        dec.set_logit_bias(token_constraints(ban=[1], bias={2: -2.0, 433: 1.5}), rows=[0, 2])
    if "grammar" in selector:
        dec.set_grammar(True, rows=[0, 1])
    if selector == "harmony":
        # Every slot's row lifts the pitches (+8: the fixture model hardly draws one by itself), and every chord row and
        # row 109 (no chord yet) ban the pitch classes 0 .. 5: slot 1 (on) may draw the other six only, slot 2 (off) any,
        # whatever the record says -- the table, its stride and the switches matter from the first draw.  Slot 0 runs the
        # grammar inside the harmony kernel.
        dec.set_logit_bias(token_constraints(ban=[1], bias={i: 8.0 for i in range(3, 131)}))
        dec.set_grammar(True, rows=[0])
        table = np.zeros((111, 16), np.float32)
        table[:110, :6] = float("-inf")
        dec.set_harmony(table, rows=[1])
    have = (dec.bias is not None, dec.gram is not None, dec.harm is not None)
    assert have == {"none": (False, False, False), "bias": (True, False, False), "grammar": (False, True, False),
                    "grammar_bias": (True, True, False), "harmony": (True, True, True)}[selector]
    uni = np.random.RandomState(5).random_sample((B, dec.ld_u)).astype(np.float32)          # the fixed uniform table
    dec.load([z["encoded_meta"].tolist()] * B, [TD._data(z, "sample8m")] * B, uni)
    return dec


@pytest.mark.parametrize("selector", SELECTORS)
def test_separate_launches_and_the_fused_launch_agree(fixture_model, selector):
    z, model = fixture_model
    with torch.no_grad():
        sep = decoder(z, model, selector)
        sep_tokens = []
        for _ in range(ITERS):
            sep.iteration()
            sep_tokens.append(sep.token.clone())
        sep.pre()                                   # (the fused launch ends with the decision of the next iteration)
        fused = decoder(z, model, selector)
        fused_tokens = []
        fused.pre()
        for _ in range(ITERS):
            fused.body_pre()
            fused_tokens.append(fused.token.clone())
    torch.cuda.synchronize()
    sep_tokens, fused_tokens = torch.stack(sep_tokens).cpu(), torch.stack(fused_tokens).cpu()
    assert torch.equal(sep_tokens, fused_tokens), (sep_tokens, fused_tokens)
    assert torch.equal(sep.fsm, fused.fsm) and torch.equal(sep.seq, fused.seq)
    assert torch.equal(sep.state.klen, fused.state.klen)
    assert int((sep_tokens >= 1).sum()) >= ITERS          # (tokens were drawn: the streams are not empty)
    assert int(sep.fsm[:, 0].min()) > 1 + len(z["encoded_meta"])          # (and appended to seq)
