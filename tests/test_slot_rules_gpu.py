"""Every rule of SLOT_RULES through the request store on the GPU: two store entries that give every rule a value of their
own, one arm launch, and the slots' control words downloaded -- in an unprimed pool (commu_decode_arm) and in a primed one
whose entry 0 starts with a memory of just over one chunk of image rows (commu_decode_arm_primed, two chunk workgroups).
The expected words are composed here, from the contracts' word functions and the order the templates were packed in."""
import pytest
import torch

import articulation_contract as AC
import density_contract as DC
import form_contract as FC
import guide_contract as GC
import interval_contract as IC
import onsets_contract as OC
import pool_contract as PC
import pool_prime_contract as PP
import voices_contract as VC

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_COND = len(PC.META)
PROMPT = 56                  # tokens of the primed entry's prompt: a memory of 65 .. 70 rows, just over one chunk of 64


def guide(pitch):
    return {"cells": 1, "bars": [[[pitch]]]}          # one bar of one cell: a block of 2 rows, shift 7


# what slot 1 holds before the arm (set by the setters, which also allocate every rule), and the two entries' requests;
# the table rules get distinct templates of one bar (the form: of two -- bar 0 of every form is free, so one-bar forms are
# all the same rows)
HELD = dict(note_order=7, voices=VC.word(3, True), density=DC.word(1, 9), interval=IC.word(5, 4), onsets=[[0]],
            guide=guide(60), articulation={"velocity": [10, 20]}, form="AB")
ENTRY0 = dict(note_order=3, voices=VC.word(2), density=DC.word(1, 4), interval=IC.word(7, 7, True), onsets=[[0, 64]],
              guide=guide(62), articulation={"velocity": [40, 80]}, form="AA")
ENTRY1 = dict(density=DC.word(2, 6), interval=IC.word(0, 12), onsets=[[32]], guide=guide(64),
              articulation={"duration": [2, 8], "within_bar": True}, form={"bars": [None, {"of": 0, "transpose": 2}]})


def words(k, **over):
    """The control words of the k-th settings packed (0: HELD, 1: ENTRY0, 2: ENTRY1): a one-row onset template and
    articulation at row k, a guide block of 2 rows at row 2 k, a form of 2 rows at row 2 k."""
    w = dict(onset=OC.word(k, 1), guide=GC.word(2 * k, 1, 7), art=AC.word(k, 1), form=FC.word(2 * k, 2))
    w.update(over)
    return w


EXPECTED = {
    1: words(0, order=7, voice=VC.word(3, True), density=DC.word(1, 9), interval=IC.word(5, 4)),            # what it held
    2: words(1, order=3, voice=VC.word(2), density=DC.word(1, 4), interval=IC.word(7, 7, True)),            # <- entry 0
    # <- entry 1: the density switches the voice word on (0: no cap) and that the note order (0: no cap)
    0: words(2, order=0, voice=0, density=DC.word(2, 6), interval=IC.word(0, 12), art=AC.word(2, 1, within_bar=True)),
}


@pytest.fixture(scope="module")
def model():
    import test_decode_slots_gpu as DS
    return DS._model(DS.NARROW, 41, eos_bias=-30.0)          # (no EOS, no Bar: a sequence runs its generation length)


@pytest.mark.parametrize("primed", [False, True], ids=["unprimed", "primed"])
def test_one_arm_moves_every_rules_word_into_its_slot(model, primed):
    import commu_amd.generate as G
    from commu_amd import ops
    data = PC.data()
    replay = None
    kw = {}
    if primed:
        gen = G.BatchedGenerator(model, torch.device(DEV), generation_length=80, memory_length=128)
        (own,), _ = gen.generate_stream(PC.META, data, 0.95, 32, need=1, accept=lambda seq, rep: seq is not None, slots=1,
                                        seed=7, max_attempts=4)
        prompt = PP.prompt_of(own, N_COND, PROMPT)
        assert len(prompt) == PROMPT
        kw = {"max_prompt": PROMPT}
    dec = G.ForcedDecoder(model, 3, 40, 128, 1.0, 1, **kw)
    if primed:
        replay, none = dec.pool_replay([PC.META] * 2, [data] * 2, [prompt, []])
        chunk = ops.decode_arm_primed_chunk_rows()
        print(f"klen0 of the primed entry: {replay['klen0']} (chunk rows {chunk})")
        assert none is None and chunk == 64 and 65 <= replay["klen0"] <= 70
    for r in G.SLOT_RULES:                                   # (the first use of every rule; slot 1's templates are packed first)
        getattr(dec, r.setter)(HELD[r.kw], rows=[1])
    klen0 = [N_COND if replay is None else replay["klen0"], N_COND]
    dec.pool_open(N_COND, grid_rows=max(klen0))
    assert dec.arm_kernel == ("commu_decode_arm_primed" if primed else "commu_decode_arm")
    dec.admit(0, PC.META, data, sampling=(0.9, 8, 1.0), primed=replay, **ENTRY0)
    dec.admit(1, PC.META, data, sampling=(0.8, 4, 0.9), **ENTRY1)
    dec.form_tok.copy_(torch.tensor([55, 77, 55], dtype=torch.int32))          # (sentinels: the arm writes -1)
    dec.state.klen.copy_(torch.tensor([40, 5, 40], dtype=torch.int32))
    dec.arm([(2, 0, None), (0, 1, None)])
    torch.cuda.synchronize()
    got = {r.stem: getattr(dec, r.ctl).cpu().tolist() for r in G.SLOT_RULES}
    for slot, want in EXPECTED.items():
        assert {stem: w[slot] for stem, w in got.items()} == want, slot
    assert dec.form_tok.cpu().tolist() == [-1, 77, -1]
    assert dec.state.klen.cpu().tolist() == [klen0[1], 5, klen0[0]]
    # (the store's words are the entries', the slots' mirrors on the host are untouched by an arm)
    P = dec._pool
    assert {r.stem: P[r.entry][:2].cpu().tolist() for r in G.SLOT_RULES} == \
        {stem: [EXPECTED[2][stem], EXPECTED[0][stem]] for stem in got}
