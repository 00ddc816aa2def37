"""One launch of the stand-alone sampling step (commu_sample_topk) from host tensors, for the GPU tests of the sampling
constraints: fills commu_sample_args field by field, so that a test names exactly the pointers it hands over -- which is
what selects the kernel (a null bias / gram / harm is the launch that never heard of it)."""
import ctypes as C

import torch

DEV = "cuda"


def sample_launch(logits, wrong, uniforms, t, k, p, v=729, active=None, logp=True, bias=None, ld_bias=None, gram=None,
                  ld_gram=None, gram_on=None, harm=None, ld_harm=None, harm_on=None, state=None, seq=None, chord_tok=None,
                  ld_seq=None, ld_chord=None, vocab=729):
    """Fresh device copies of everything, one launch, the results on the host: (logits as written back, token, probs_out,
    logp_out or None).  t / k / p: a number for all rows or a tensor [n] (the *_rows arrays); every other tensor argument:
    None passes a null pointer; ld_*: a row stride to pass instead of the tensor's own.  Before the launch token holds -7,
    probs_out ([n][vocab]) -3.0 and logp_out 7.0."""
    from commu_amd._lib import SampleArgs, call, struct_args
    n = logits.shape[0]
    dev = lambda x: None if x is None else torch.as_tensor(x).to(DEV).contiguous()
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    ld = lambda x, given=None: given if given is not None else (0 if x is None else x.stride(0))
    lg = logits.clone().to(DEV)
    pr = torch.full((n, vocab), -3.0, device=DEV)
    tok = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((n, 2), 7.0, device=DEV) if logp else None
    rows = [dev(x) if isinstance(x, torch.Tensor) else None for x in (t, k, p)]
    held = [dev(x) for x in (wrong, uniforms, active, bias, gram, gram_on, harm, harm_on, state, seq, chord_tok)]
    w, u, a, bd, gd, god, hd, hod, st, sq, ct = held
    args = struct_args(
        SampleArgs, logits=ptr(lg), ld=lg.stride(0), nseq=n, V=v, wrong=ptr(w), ldw=ld(w), uniforms=ptr(u), active=ptr(a),
        temperature=0.0 if rows[0] is not None else t, top_k=1 if rows[1] is not None else k,
        top_p=1.0 if rows[2] is not None else p, temperature_rows=ptr(rows[0]), top_k_rows=ptr(rows[1]),
        top_p_rows=ptr(rows[2]), token=ptr(tok), probs_out=ptr(pr), ldp=pr.stride(0), logp_out=ptr(lp),
        bias=ptr(bd), ld_bias=ld(bd, ld_bias), gram=ptr(gd), ld_gram=ld(gd, ld_gram), gram_on=ptr(god),
        harm=ptr(hd), ld_harm=ld(hd, ld_harm), harm_on=ptr(hod), state=ptr(st), seq=ptr(sq), ld_seq=ld(sq, ld_seq),
        chord_tok=ptr(ct), ld_chord=ld(ct, ld_chord))
    call("commu_sample_topk", C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    del held, rows
    return lg.cpu(), tok.cpu(), pr.cpu(), None if lp is None else lp.cpu()
