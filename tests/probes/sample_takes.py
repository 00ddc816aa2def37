"""What the take rows of the form rule (commu_decode_loop_args.form_src) cost, and whether the paths that exist moved: the
fused loop launch alone (commu_decode_sample_post_pre, 64 rows, no model step), 200 launches back to back in a captured graph,
by HIP events, every window from the same restored state -- the method and the worlds of sample_form.py --rows kernel:

  null              -- without the form arguments: the kernel of a decoder that never got a form;
  form_off          -- the form kernel with every word off;
  form_replay_own   -- every slot inside a replay bar of its OWN past (the next group in the first chunk);
  form_replay_take  -- every slot inside a replay bar of a TAKE: the same groups, read from form_src; a tree from before the
                       take rows (its argument struct has no form_src) runs the first three only.

To compare with the parent run the probe from two trees IN TURN, each process on its own (--pkg DIR, --tag NAME), several
times alternating: the spread between the processes of one tree is the resolution of the comparison.

JSON lines.    python tests/probes/sample_takes.py [--pkg DIR] [--tag NAME] [--out FILE]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sample_harm as SH  # noqa: E402
import sample_voices as SV  # noqa: E402

B, REPS = SV.B, SV.REPS
N = 200
LD = 8192
TAKE_BIT = 1 << 7


def kernel_rows(dev, tag):
    import ctypes as C

    import torch
    from commu_amd import _lib
    from commu_amd._lib import call, struct_args
    NF, NS = call("commu_forcing_state_ints"), call("commu_form_state_ints")
    has_src = "form_src" in [n for n, _ in _lib.DecodeLoopArgs._fields_]
    i32, u8 = torch.int32, torch.uint8
    logits = torch.randn(B, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2.5
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    source = []
    for i in range(N // 4 + 2):
        source += [434 + i % 90, 150, 40 + i % 40, 304]
    head_len = 1 + len(SH.META)
    body = [0] + SH.META + [2, 432, 199] + source + [2, 432, 285]
    chord_tok = torch.full((B, 64), 199, dtype=i32, device=dev)
    chord_pos = torch.full((B, 64), 432, dtype=i32, device=dev)
    wrong = torch.zeros(B, 729, dtype=u8, device=dev)
    utable = torch.rand(B, N + 8, device=dev)
    tok = torch.zeros(B, dtype=torch.long, device=dev)
    active, keep, draw = (torch.zeros(B, dtype=u8, device=dev) for _ in range(3))
    uni = torch.rand(B, device=dev)
    token = torch.zeros(B, dtype=i32, device=dev)
    work = logits.clone()
    modes, alive = {}, []

    def add(name, form, replay):
        seq = torch.zeros(B, LD, dtype=i32, device=dev)
        seq[:, :len(body)] = torch.tensor(body, dtype=i32, device=dev)
        fsm = torch.zeros(B, NF, dtype=i32, device=dev)
        # len, forced, redo, first, filled, done, failed, iters, nbar, nchord, cur, length_fit, ndraw, ntrace
        fsm[:] = torch.tensor([len(body), -1, 0, 0, 1, 0, 0, 0, 2, 64, 2, 1, 0, 0], dtype=i32, device=dev)
        kw, state = {}, None
        bufs = [fsm, seq, wrong, work, tok, active, keep, draw, uni]
        if form:
            state = torch.zeros(B, NS, dtype=i32, device=dev)
            state[:, 5] = -1
            table = torch.zeros(4096, 4, dtype=i32, device=dev)
            row = 64 << 8
            if replay == "own":      # (active, cursor behind the source bar's BAR, end at the next BAR, phase 0, the row, no group)
                state[:, :6] = torch.tensor([1, head_len + 1, head_len + 3 + len(source), 0, row, -1], dtype=i32, device=dev)
            if replay == "take":     # (the same groups in the take buffer, behind one BAR)
                src = torch.tensor([2, 432, 199] + source + [2], dtype=i32, device=dev)
                row |= TAKE_BIT
                state[:, :6] = torch.tensor([1, 1, 3 + len(source), 0, row, -1], dtype=i32, device=dev)
                table[1, 1], table[1, 2] = 1, 3 + len(source)
                kw.update(form_src=p(src), form_src_len=int(src.numel()))
                alive.append(src)
            table[1, 0] = row
            ctl = torch.full((B,), 2 * 4096 if replay else -1, dtype=i32, device=dev)
            ftok = torch.full((B,), -1, dtype=i32, device=dev)
            kw.update(form_ctl=p(ctl), form_table=p(table), form_rows=4096, form_state=p(state), form_tok=p(ftok))
            bufs += [state, ftok]
            alive.extend([ctl, table])
        draw.fill_(0 if replay else 1)
        keep.fill_(1)
        a = struct_args(_lib.DecodeLoopArgs, logits=p(work), ld=768, V=729, B=B, wrong=p(wrong), temperature=0.95, top_k=32,
                        top_p=1.0, token=p(token), state=p(fsm), seq=p(seq), ld_seq=LD, chord_tok=p(chord_tok),
                        chord_pos=p(chord_pos), ld_chord=64, utable=p(utable), ld_u=N + 8, max_iters=1 << 30, tok=p(tok),
                        active=p(active), keep=p(keep), draw=p(draw), uni=p(uni), lmax=1 << 30, **kw)
        saved = [t.clone() for t in bufs]

        def launches():
            for _ in range(N):
                call("commu_decode_sample_post_pre", C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launches()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            launches()
        modes[name] = (g, bufs, saved, a, fsm, seq, state)
    add("null", False, None)
    add("form_off", True, None)
    add("form_replay_own", True, "own")
    if has_src:
        add("form_replay_take", True, "take")
    us = {m: [] for m in modes}
    info = {}
    for rep in range(REPS + 1):
        for m in modes:
            g, bufs, saved, a, fsm, seq, state = modes[m]
            for dst, src in zip(bufs, saved):
                dst.copy_(src)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            torch.cuda.synchronize()
            if rep:
                us[m].append(1e3 * s.elapsed_time(e) / N)
            info[m] = {"done": int(fsm[:, 5].sum()), "drawn": int(fsm[:, 12].sum()),
                       "replaying": None if state is None else int(state[:, 0].sum()),
                       "appended": int(fsm[0, 0]) - len(body)}
    # the two replay modes hand out the same tokens
    if has_src:
        n = int(modes["form_replay_own"][4][0, 0])
        assert n > len(body) + N // 2 and bool((modes["form_replay_own"][5][:, :n] == modes["form_replay_take"][5][:, :n]).all())
    return {"what": "fused loop launch alone, 200 launches back to back", "tree": tag, "rows": B, "after_the_window": info,
            "us_per_launch_graph_replay": {m: SH.spread(us[m], 3) for m in us}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", type=str, default=os.path.join(SH.ROOT, "commu-code_amd"))
    ap.add_argument("--tag", type=str, default="this tree")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    with torch.no_grad():
        r = kernel_rows(torch.device("cuda"), a.tag)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
