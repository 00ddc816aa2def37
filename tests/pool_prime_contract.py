"""Shared builders of the primed request-pool tests (tests/test_pool_prime_host.py, tests/test_pool_prime_gpu.py): the
primed arm launch's (commu_decode_arm_primed, include/commu_hip.h) view of pool_contract's one restatement and one case
builder, and the helpers of the end-to-end tests."""
import pool_contract as PC

NF = PC.NF


def arm_primed_expected(before, store, images, jobs, variates, B, R, Lmax, img_rows, ld_head, ring=False, grid_rows=0):
    """What the primed launch must leave: pool_contract.arm_restated (its operands are described there) with the sequence
    head copied up to the record's length word."""
    return PC.arm_restated(before, store, images, jobs, variates, B, R, Lmax, img_rows, ld_head, ring=ring,
                           grid_rows=grid_rows)


def prime_case(torch, kv, DH, klen0, lens, B=5, Lmax=200, R=3, img_rows=144, ld_seq=60, ld_head=48, e_trace=True, **kw):
    """pool_contract.case for the primed launch: images of img_rows rows, sequence heads of ld_head words, a trace twin."""
    return PC.case(torch, kv, DH, klen0, lens, True, B=B, Lmax=Lmax, R=R, img_rows=img_rows, ld_seq=ld_seq, ld_head=ld_head,
                   e_trace=e_trace, **kw)


def expected(c, before, jobs, variates):
    """arm_primed_expected for a prime_case."""
    return PC.arm_expected(c, before, jobs, variates)


def prompt_of(seq, n_cond, k):
    """The first k tokens after [0] + meta of a sequence the model generated (fewer where it is shorter; its last token,
    EOS, never)."""
    body = list(seq[1 + n_cond:-1])
    return body[:k]
