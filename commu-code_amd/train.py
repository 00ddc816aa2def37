#!/usr/bin/env python3
"""Training driver with the reference's command line (train.py:57-70: --data_dir --work_dir --local_rank):

    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 commu-code_amd/train.py \\
        --data_dir <output_npy> --work_dir <dir>            (one process per MI355X, RCCL over xGMI)
    python commu-code_amd/train.py --data_dir <output_npy> --work_dir <dir>            (single GPU)

What the reference's script does at import time and in train() (:113-288, :357-484) is done here in `main`:
run directory agreed on by a broadcast (C2), per-rank seeds / shuffle seeds / LR scaling (Q7, Q9), the packed-stream
batch iterator, the train step (commu_amd.train.Trainer: micro-batches, clip, Adam, inverse-sqrt LambdaLR, ONE
gradient all-reduce per optimiser step overlapped with backward), the logging window (one packed all-reduce, C5),
evaluation every `eval_interval` steps with the same_length / long-memory setting (C6) and checkpoint_last /
checkpoint_best written by rank 0 between barriers (C7).  The reference's hyper-parameters are hard-coded defaults
(config_helper.py:4-49); the extra flags below only exist so that small runs and the benchmark shapes can be driven
from the same entry point.  Fine-tuning flags (not in the reference either): --init_checkpoint / --resume, --lr,
--warmup_step, --weight_decay, --adamw and --param_groups (per-tensor lr multiplier / weight decay / frozen, see
commu_amd.optim.resolve_groups); what can be refused without a dataset or a model is refused first (check_fine_tune_args).
Loss options (not in the reference): --label_smoothing, --z_loss (the fused loss kernels of the training step; evaluation and
the logs keep reporting the plain NLL) and --report_families (per-family validation NLL); refused first likewise
(check_loss_args).  A checkpoint stores the position of the training batch stream, and --resume continues from it.
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="ComMU Transformer-XL training on MI355X")
    p.add_argument("--data_dir", type=str, required=True, help="location of the data corpus (output_npy)")
    p.add_argument("--local_rank", type=int, default=int(os.environ.get("LOCAL_RANK", 0)))
    p.add_argument("--work_dir", type=str, required=True, help="Base directory to save the trained model.")
    # -- not in the reference: overrides of its hard-coded defaults
    p.add_argument("--no-merge-chunks", dest="merge_chunks", action="store_false", default=None,
                   help="(not in the reference) run the batch_chunk micro-batches one after the other like the reference; "
                        "default: one forward / backward over all columns with per-micro-batch loss weights when the batch "
                        "has at most 65536 tokens (same loss and gradients)")
    p.add_argument("--graph", action="store_true",
                   help="replay the optimiser step from hipGraphs once its shapes are steady (not in the reference; pays "
                        "when a micro-batch is small enough for the host's launch rate to bound the step)")
    p.add_argument("--parity", action="store_true",
                   help="(not in the reference) train in the reference's fp32 arithmetic: fp32 forward with dropout, fp32 "
                        "backward, eager steps (model.fp32_training + model.parity_fp32; evaluation in fp32 too); "
                        "--label_smoothing and --z_loss apply to it as well (the fp32 loss kernels)")
    p.add_argument("--max_step", type=int, default=None)
    p.add_argument("--log_interval", type=int, default=None)
    p.add_argument("--eval_interval", type=int, default=None)
    for name in ("num_layers", "num_heads", "units", "inner_size", "tgt_length", "mem_length", "batch_size",
                 "batch_chunk"):
        p.add_argument("--" + name, type=int, default=None)
    # -- not in the reference: fine-tuning (start from a checkpoint, weight decay, per-tensor optimiser groups)
    p.add_argument("--init_checkpoint", type=str, default=None, metavar="FILE",
                   help="(not in the reference) start from the MODEL WEIGHTS of a checkpoint (strict=False, as the "
                        "generation loader reads it); the optimiser is fresh and the step starts at 0")
    p.add_argument("--resume", type=str, default=None, metavar="FILE",
                   help="(not in the reference) continue a run: model, optimiser, scheduler, train_step and best_val_loss of "
                        "a checkpoint, and the batch stream from the stored seed, epoch and batch index (same number of ranks, "
                        "batch size, tgt_length and corpus).  Otherwise, and for a checkpoint without a stored position, the "
                        "resumed run draws a fresh shuffle from "
                        "seed + 1000 * rank + train_step")
    p.add_argument("--lr", type=float, default=None, help="(not in the reference) overrides TRAIN.lr")
    p.add_argument("--warmup_step", type=int, default=None, help="(not in the reference) overrides TRAIN.warmup_step")
    p.add_argument("--weight_decay", type=float, default=None,
                   help="(not in the reference) overrides TRAIN.weight_decay (torch.optim.Adam's coupled decay)")
    p.add_argument("--adamw", action="store_true",
                   help="(not in the reference) decoupled weight decay as in torch.optim.AdamW")
    p.add_argument("--param_groups", type=str, default=None, metavar="SPEC",
                   help="(not in the reference) JSON text or a JSON file: a list of {\"match\": glob or list of globs over the "
                        "state-dict names, \"lr_mult\": 1, \"weight_decay\": the default, \"frozen\": false}; the first "
                        "match wins, unmatched tensors keep the defaults")
    # -- not in the reference: loss options of the training step, per-family validation report
    p.add_argument("--label_smoothing", type=float, default=None, metavar="EPS",
                   help="(not in the reference) overrides TRAIN.label_smoothing: train on (1 - EPS) nll + EPS * cross entropy "
                        "against the uniform distribution over the vocabulary, 0 <= EPS < 1 (evaluation and the logs report "
                        "the plain nll)")
    p.add_argument("--z_loss", type=float, default=None, metavar="ZETA",
                   help="(not in the reference) overrides TRAIN.z_loss: adds ZETA * logsumexp(logits)^2 per token to the "
                        "training loss, ZETA >= 0")
    p.add_argument("--report_families", action="store_true", default=None,
                   help="(not in the reference) overrides TRAIN.report_families: every evaluation also logs the nll and the "
                        "token count per token family (pad/EOS/Bar, position, chord, velocity, pitch, duration, meta, "
                        "other); checkpoint_best.pt keeps the report under \"val_families\"")
    return p.parse_args(argv)


def check_fine_tune_args(args):
    """The refusals that need neither a dataset nor a model; returns the parsed --param_groups (or None)."""
    from commu_amd.optim import GroupSpecError, load_group_spec
    if args.init_checkpoint is not None and args.resume is not None:
        raise ValueError("--init_checkpoint and --resume exclude each other: the first starts a new run from a "
                         "checkpoint's weights, the second continues the checkpoint's own run")
    for flag in ("init_checkpoint", "resume"):
        path = getattr(args, flag)
        if path is not None and not os.path.isfile(path):
            raise ValueError(f"--{flag}: no such file: {path}")
    for flag in ("lr", "weight_decay"):
        x = getattr(args, flag)
        if x is not None and not (0.0 <= x < float("inf")):
            raise ValueError(f"--{flag} {x} must be a finite number >= 0")
    if args.param_groups is None:
        return None
    try:
        return load_group_spec(args.param_groups)
    except GroupSpecError as exc:
        raise ValueError(f"--param_groups: {exc}") from None


def check_loss_args(args):
    """The refusals of the loss options that need neither a dataset nor a model."""
    from commu_amd.model.model import check_loss_options
    eps, zeta = getattr(args, "label_smoothing", None), getattr(args, "z_loss", None)
    try:
        check_loss_options(0.0 if eps is None else eps, 0.0 if zeta is None else zeta)
    except ValueError as exc:
        raise ValueError(f"--label_smoothing / --z_loss: {exc}") from None


def main(argv=None):
    from commu_amd.ddp import GradReducer
    from commu_amd.model.config_helper import get_default_cfg_training
    from commu_amd.model.dataset import ComMUDataset
    from commu_amd.train import (Trainer, build_model, evaluate_best_checkpoint, load_checkpoint, read_checkpoint,
                                 resume_position, save_checkpoint, stream_key)
    args = parse_args(argv)
    group_spec = check_fine_tune_args(args)
    check_loss_args(args)
    cfg = get_default_cfg_training()
    cfg.defrost()
    for name in ("num_layers", "num_heads", "units", "inner_size"):
        if getattr(args, name) is not None:
            cfg.MODEL[name] = getattr(args, name)
    for name in ("tgt_length", "mem_length", "batch_size", "batch_chunk", "max_step", "log_interval", "eval_interval"):
        if getattr(args, name) is not None:
            cfg.TRAIN[name] = getattr(args, name)
    for name in ("lr", "warmup_step", "weight_decay", "label_smoothing", "z_loss", "report_families"):
        if getattr(args, name) is not None:
            cfg.TRAIN[name] = getattr(args, name)
    cfg.freeze()
    torch.cuda.set_device(args.local_rank)
    device = torch.device("cuda", args.local_rank)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", init_method="env://")          # train.py:361 (RCCL on ROCm)
    rank = dist.get_rank() if world > 1 else 0
    # C2: every rank writes into the run directory named after rank 0's clock (train.py:363-370)
    exp_time = torch.tensor(time.time(), dtype=torch.float64, device=device)
    if world > 1:
        dist.broadcast(exp_time, 0)
    work_dir = os.path.join(args.work_dir, time.strftime("%Y%m%d-%H%M%S", time.localtime(float(exp_time))))
    os.makedirs(work_dir, exist_ok=True)
    if rank == 0:
        with open(os.path.join(work_dir, "config.yml"), "w") as f:
            f.write(str(cfg))

    def log(msg):
        if rank == 0:
            print(msg, flush=True)
        with open(os.path.join(work_dir, f"train_rank{rank}.log"), "a") as f:
            f.write(msg + "\n")

    seed = cfg.TRAIN.seed
    np.random.seed(seed)
    torch.manual_seed(seed)
    dataset = ComMUDataset(args.data_dir, cfg)
    num_gpus = world                                                            # train.py:395 (one process per GPU)
    assert cfg.TRAIN.batch_size % num_gpus == 0
    batch_size = cfg.TRAIN.batch_size // num_gpus
    assert batch_size % cfg.TRAIN.batch_chunk == 0
    stream_seed = seed + 1000 * rank                                            # Q9
    train_iter = dataset.get_iterator(batch_size, cfg.TRAIN.tgt_length, device, "train", True, seed=stream_seed)
    key = stream_key(num_gpus, batch_size, cfg.TRAIN.tgt_length, dataset.train_seq_length)
    val_iter = dataset.eval_iterator(cfg.EVALUATE.batch_size, cfg.EVALUATE.tgt_length, device, "valid",
                                     local_rank=rank, world_size=num_gpus)
    test_iter = dataset.eval_iterator(cfg.EVALUATE.batch_size, cfg.EVALUATE.tgt_length, device, "test",
                                      local_rank=rank, world_size=num_gpus)
    assert cfg.MODEL.units % cfg.MODEL.num_heads == 0
    model = build_model(cfg, dataset.vocab, device)
    if args.init_checkpoint is not None:
        missing, unexpected = model.load_state_dict(read_checkpoint(args.init_checkpoint)["model"], strict=False)
    if getattr(args, "parity", False):
        model.fp32_training = True
        model.parity_fp32 = True
    model.loss_options = {"label_smoothing": cfg.TRAIN.label_smoothing, "z_loss": cfg.TRAIN.z_loss}
    log(f"#total params = {sum(p.nelement() for p in model.parameters())}")
    if args.init_checkpoint is not None:
        log(f"weights of {args.init_checkpoint} (missing: {list(missing)}, unexpected: {list(unexpected)})")
    reducer = GradReducer() if world > 1 else None
    if reducer is not None:
        reducer.broadcast_params(model)                                         # DDP constructor semantics (C3)
    trainer = Trainer(model, cfg, num_gpus=num_gpus, reducer=reducer, graph=bool(getattr(args, "graph", False)),
                      merge_chunks=getattr(args, "merge_chunks", None), settle_heap=True, param_groups=group_spec,
                      decoupled=bool(args.adamw))
    best_val_nll = float("inf")
    if args.resume is not None:
        # (a checkpoint whose optimiser grouping differs from these flags is refused by FusedAdam.load_state_dict)
        ck = read_checkpoint(args.resume)
        trainer.train_step, best = load_checkpoint(args.resume, model, trainer.optimizer, trainer.scheduler, ck=ck)
        best_val_nll = float("inf") if best is None else float(best)
        trainer._log_step0 = trainer.train_step                                 # the logging window starts here
        if reducer is not None:
            reducer.broadcast_params(model)
        log(f"resumed {args.resume} at step {trainer.train_step}")
        if trainer.train_step >= cfg.TRAIN.max_step:
            raise ValueError(f"--resume: the checkpoint is at step {trainer.train_step}, max_step is {cfg.TRAIN.max_step}")
        found = resume_position(ck, rank, key)
        if found is not None:          # the stream of the checkpoint's run, from the batch after its last step
            stream_seed, start = found
            train_iter = dataset.get_iterator(batch_size, cfg.TRAIN.tgt_length, device, "train", True, seed=stream_seed,
                                              start=start)
            log(f"batch stream resumed at epoch {start[0]}, batch {start[1]} (stream seed {stream_seed})")
        else:          # no position in the checkpoint, or one of another stream layout: a fresh shuffle
            stream_seed = seed + 1000 * rank + trainer.train_step
            train_iter = dataset.get_iterator(batch_size, cfg.TRAIN.tgt_length, device, "train", True, seed=stream_seed)
        del ck

    def data_position():
        """stream_key + {"streams": [seed, epoch, index] of every rank}: the seed each rank's stream was really drawn from
        (after a fresh shuffle on resume that is not seed + 1000 * rank) -- one packed all-reduce, each rank fills its slots"""
        own = train_iter.position
        slots = [0.0] * (3 * num_gpus)
        slots[3 * rank:3 * rank + 3] = float(stream_seed), float(own["epoch"]), float(own["index"])
        if reducer is not None:
            slots = reducer.sum_scalars(slots, device=device)
        return dict(key, streams=[[int(x) for x in slots[3 * r:3 * r + 3]] for r in range(num_gpus)])

    def checkpoint(name, val_nll, val_families=None):                           # train.py:29-54 (C7)
        position = data_position()
        if reducer is not None:
            reducer.barrier()
        if rank == 0:
            save_checkpoint(os.path.join(work_dir, name), model, trainer.optimizer, dataset.vocab, trainer.train_step,
                            val_nll, trainer.scheduler, data_position=position, val_families=val_families)
        if reducer is not None:
            reducer.barrier()

    log("Start training")
    t_log = time.time()
    for data, target, reset_mems, ntok in train_iter():
        trainer.step(data, target, reset_mems, ntok)
        step = trainer.train_step
        if step % cfg.TRAIN.log_interval == 0:
            nll, gnorm, tokens = trainer.log_window()
            elapsed = time.time() - t_log
            log("Train Step {}/{}, lr={:f}, tokens/s={:.1f}, nll={:.4f}, ppl={:.2f}, grad norm={}, ".format(
                step, cfg.TRAIN.max_step, trainer.optimizer.param_groups[0]["lr"], tokens / elapsed, nll,
                math.exp(min(nll, 50.0)), gnorm))
            t_log = time.time()
        if step % cfg.TRAIN.eval_interval == 0:
            t0 = time.time()
            fam = {} if cfg.TRAIN.report_families else None
            val_tok, val_nll = trainer.evaluate_reduced(val_iter, families=fam)
            msg = "Eval step {}, time={}s, val nll={}, val ppl={},".format(step, time.time() - t0, val_nll,
                                                                          math.exp(min(val_nll, 50.0)))
            if fam is not None:
                msg += " families: " + ", ".join(f"{k} nll={v['nll']:.4f} tokens={v['tokens']}" for k, v in fam.items())
            log(msg)
            checkpoint("checkpoint_last.pt", val_nll)
            if val_nll < best_val_nll:
                best_val_nll = val_nll
                checkpoint("checkpoint_best.pt", best_val_nll, val_families=fam)
                t0 = time.time()
                test_tok, test_nll = trainer.evaluate_reduced(test_iter)
                log("Test step {}, time={}s, test nll={}, test ppl={}, #evaluated tokens={}".format(
                    step, time.time() - t0, test_nll, math.exp(min(test_nll, 50.0)), test_tok))
            t_log = time.time()
        if step >= cfg.TRAIN.max_step:
            log("-" * 100)
            log("End of training")
            break
    # train.py:486-513: the best checkpoint, reloaded into a fresh same_length model, on the test split
    best = os.path.join(work_dir, "checkpoint_best.pt")
    if reducer is not None:
        reducer.barrier()
    if os.path.exists(best):
        test_nll, _ = evaluate_best_checkpoint(best, cfg, dataset.vocab, device, test_iter, reducer=reducer,
                                               parity=bool(getattr(args, "parity", False)))
        log("=" * 100)
        log("| End of training | test nll {:5.2f} | test ppl {:9.3f}".format(test_nll, math.exp(min(test_nll, 50.0))))
        log("=" * 100)
    if world > 1:
        dist.destroy_process_group()
    return work_dir


if __name__ == "__main__":
    main()
