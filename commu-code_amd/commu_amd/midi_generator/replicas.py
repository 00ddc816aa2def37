"""Generation replicas: `num_generate` independent sequences split across GPUs, one process per GPU, no collective
(the reference generates them one after the other on one device, midi_inferrer.py:338-354).
Lives in the package (not in the generate.py script) so that spawned replica processes can import the worker."""
from __future__ import annotations


def split_num_generate(num_generate, n_replicas):
    """Shares of `num_generate` for `n_replicas` independent replicas (first ones take the remainder)."""
    n_replicas = max(1, min(int(n_replicas), int(num_generate)))
    base, rem = divmod(int(num_generate), n_replicas)
    return [base + (1 if r < rem else 0) for r in range(n_replicas)]


def logprobs_to_lists(logprobs):
    """Log-probability arrays ([len, 2] float32, NaN rows where a token was not drawn) as JSON-ready lists: one list of
    [full, kept] pairs per sequence, None for the entries that were not drawn."""
    import math
    return [None if lp is None else [None if math.isnan(f) or math.isnan(k) else [f, k] for f, k in lp.tolist()]
            for lp in logprobs]


def generate_on_device(model_args, in_args, device_index, num_generate, uniform_seed, max_rounds, training_cfg=None,
                       logprobs=False, prompt=None, logit_bias=None, harmony=None, class_sampling=None):
    """One replica: checkpoint -> model on cuda:<device_index>, `num_generate` validated sequences (logprobs: and their
    log-probabilities as logprobs_to_lists gives them, a third value).  prompt: token ids every sequence continues.
    logit_bias: a constraint row (generate.token_constraints, a numpy array) on what every sequence may draw.
    harmony: a harmony table (generate.harmony_rows, a numpy array) -- drawn pitches are weighed by the sounding chord.
    class_sampling: a class-control table (generate.class_sampling, a numpy array); the command line's --class_sampling
    travels in model_args instead.
    model_args carries the decode options of every replica (--parity, --sliding_memory, --kv_cache, --share_prompt,
    --decode_slots, --class_sampling, ...): they reach
    the generator through the inference configuration that ModelInitializeTask builds."""
    import copy

    import torch
    from commu_amd.midi_generator.meta import PreprocessTask
    from commu_amd.midi_generator.midi_inferrer import InferenceTask
    from commu_amd.midi_generator.model_initializer import ModelInitializeTask
    torch.cuda.set_device(device_index)
    device = torch.device("cuda", device_index)
    init = ModelInitializeTask(model_args, map_location="cpu", device=device, training_cfg=training_cfg)
    model = init.execute()
    pre = PreprocessTask()
    args = copy.deepcopy(in_args)
    args["num_generate"] = num_generate
    encoded_meta = pre.execute(args)
    task = InferenceTask(device)
    task.uniform_seed = uniform_seed
    task(model=model, input_data=pre.input_data, inference_cfg=init.inference_cfg)
    if logprobs:
        seqs, lps = task.execute(encoded_meta, max_rounds=max_rounds, return_logprobs=True, prompt=prompt,
                                 logit_bias=logit_bias, harmony=harmony, class_sampling=class_sampling)
        return encoded_meta, seqs, logprobs_to_lists(lps)
    return encoded_meta, task.execute(encoded_meta, max_rounds=max_rounds, prompt=prompt, logit_bias=logit_bias,
                                      harmony=harmony, class_sampling=class_sampling)


def generate_requests_on_device(model_args, requests, device_index, training_cfg=None, logprobs=False, harmony=None):
    """generate.py --requests: checkpoint -> model on cuda:<device_index>, then every request (a dict of one request's
    input arguments plus seed, max_rounds, its constraint row logit_bias, its prompt_tokens, its onsets template, its guide track, its articulation and its form) through PreprocessTask and all of them in ONE
    pool (InferenceTask.execute_pool).  Returns one dict per request in list order: encoded_meta, sequences, attempts
    (and logprobs as logprobs_to_lists gives them)."""
    import torch
    from commu_amd.midi_generator.meta import PreprocessTask
    from commu_amd.midi_generator.midi_inferrer import InferenceTask
    from commu_amd.midi_generator.model_initializer import ModelInitializeTask
    torch.cuda.set_device(device_index)
    device = torch.device("cuda", device_index)
    init = ModelInitializeTask(model_args, map_location="cpu", device=device, training_cfg=training_cfg)
    model = init.execute()
    items = []
    for r in requests:
        pre = PreprocessTask()
        args = {k: v for k, v in r.items() if k not in ("seed", "max_rounds", "logit_bias", "prompt_tokens", "onsets", "guide",
                                                       "articulation", "form")}
        encoded_meta = pre.execute(args)
        items.append({"encoded_meta": encoded_meta, "input_data": pre.input_data, "seed": int(r.get("seed") or 0),
                      "max_rounds": r.get("max_rounds"), "logit_bias": r.get("logit_bias"),
                      "prompt": r.get("prompt_tokens"), "onsets": r.get("onsets"), "guide": r.get("guide"),
                      "articulation": r.get("articulation"), "form": r.get("form")})
    task = InferenceTask(device)
    task(model=model, input_data=None, inference_cfg=init.inference_cfg)
    res = task.execute_pool(items, return_logprobs=logprobs, harmony=harmony)
    out = []
    for it, r in zip(items, res):
        doc = {"encoded_meta": it["encoded_meta"], "sequences": r.sequences, "attempts": r.attempts_started}
        if logprobs:
            doc["logprobs"] = logprobs_to_lists(r.logprobs)
        out.append(doc)
    return out


def replica_worker(rank, device_index, model_args, in_args, share, max_rounds, training_cfg, q, logprobs=False,
                   prompt=None, logit_bias=None, harmony=None, class_sampling=None):
    try:
        # distinct variates per replica: 1_000_003 apart (a replica's rounds / sequences use seed + 7919 r + b)
        q.put((rank, generate_on_device(model_args, in_args, device_index, share, 1_000_003 * rank, max_rounds,
                                        training_cfg, logprobs, prompt, logit_bias, harmony, class_sampling)))
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))
