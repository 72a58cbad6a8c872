"""Shared training harness behind train.py (MultiModalVAE), train_dna2rna.py and train_rna2dna.py.

Loop shape = the reference's trainers (train_dna2rna.py:72-252; optimize_hyperparameters.py:163-211 for MultiModalVAE):
AdamW(lr, weight_decay) + ReduceLROnPlateau(min, factor, patience) + beta warm-up + per-epoch validation + best-checkpoint
`torch.save(model.state_dict())` + early stopping + `latest_*_run_id.txt`.  What is different is HOW a step runs on the MI355X:

  * the dataset lives in HBM; an epoch is a device permutation, a minibatch is ONE gather launch (mmvae_gather_rows) through a
    static index vector -- the reference builds every sample with `torch.tensor(row)` in Python (src/data/dataset.py:28-39);
  * the whole step [gather, forward, loss, backward, AdamW] is one hipGraph replay (mmvae.graphs.GraphedTrainStep); beta and the
    learning rate live in device scalars, so the warm-up and the LR scheduler need no re-capture;
  * the loss floats of every step reach the host one step late (pinned 20-byte copies), so the host never stalls the GPU;
  * under torchrun every rank owns an equal row shard, gradients are SUM-all-reduced (RCCL) between the two graph replays,
    BatchNorm running statistics and the validation loss are averaged over ranks before any control-flow decision.
  * `--resume state.pt` continues a run (model + optimiser + scheduler + Philox position + epoch counters): the reference
    cannot resume (it only saves model weights).
"""
import argparse
import os
import time
from datetime import datetime

import torch
import torch.distributed as dist

import hostlib
from mmvae import parallel, checkpoint
from mmvae.data import balanced_class_weights, load_matched, load_pickled_dataset, split_indices, synthetic_dataset  # noqa: F401  (re-exported)
from mmvae.graphs import GraphedTrainStep
from mmvae.optim import FusedAdamW
from src.config import Config
from src.models import KINDS, forward_loss, make_model  # noqa: F401  (KINDS: re-exported)


def build_parser(kind):
    ap = argparse.ArgumentParser(description=f"{KINDS[kind]['title']} trainer on MI355X")
    hostlib.add_dataset_args(ap)
    hostlib.add_model_args(ap, n_sites=True)
    ap.add_argument("--batch-size", type=int, default=4096, help="rows per GPU")
    ap.add_argument("--epochs", type=int, default=Config.NUM_EPOCHS)
    hostlib.add_precision_args(ap, input_dtype_help=hostlib.INPUT_DTYPE_HELP + ": bf16 converts them ONCE (mmvae.to_bf16_rows, padded bf16 "
                               "rows); the first-layer GEMMs, their dW GEMMs and the reconstruction losses then read 2 bytes per element")
    ap.add_argument("--checkpoint-dir", default=Config.CHECKPOINT_DIR)
    ap.add_argument("--resume", default=None, help="training state written by --save-state (model + optimiser + scheduler + noise)")
    ap.add_argument("--save-state", default=None, help="write a resumable training state here after every epoch")
    ap.add_argument("--eager", action="store_true", help="issue every launch from Python (reference-shaped loop) instead of the captured step")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend under torchrun (nccl = RCCL; gloo only for rehearsals)")
    ap.add_argument("--single-device", action="store_true", help="rehearsal: every rank on cuda:0 (needs --backend gloo)")
    ap.add_argument("--log-json", default=None, help="append one JSON object per epoch (steps, train/val loss, lr, early-stop counter) to "
                                                     "<path>.rank<r>: every rank writes its own file, so that a run can be checked for identical decisions")
    return ap


def run(kind, argv=None):
    args = build_parser(kind).parse_args(argv)
    tag = KINDS[kind]["tag"]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("the trainers need an MI355X: the product path has no CPU fallback")
    if args.single_device:
        if args.backend == "nccl":
            raise SystemExit("--single-device puts every rank on cuda:0, which RCCL refuses: use --backend gloo")
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    tpm, beta_v, site, (args.input_dim_a, args.input_dim_b, args.n_sites) = load_matched(
        args.data, args.samples, args.input_dim_a, args.input_dim_b, args.n_sites, Config.RANDOM_SEED)
    n = tpm.shape[0]
    val_idx, train_idx = split_indices(n)
    lo, hi = parallel.shard_rows(train_idx.numel(), rank, world, equal=True)   # equal shards: every rank runs the same number of steps
    tr = [t[train_idx[lo:hi]].to(dev).contiguous() for t in (tpm, beta_v, site)]
    va = [t[val_idx].to(dev).contiguous() for t in (tpm, beta_v, site)]
    if args.input_dtype == "bf16":                                              # bf16 storage: one conversion per run, not per step
        from mmvae import to_bf16_rows
        tr[:2] = [to_bf16_rows(t) for t in tr[:2]]
        va[:2] = [to_bf16_rows(t) for t in va[:2]]
    class_weights = balanced_class_weights(site[train_idx], args.n_sites).to(dev) if kind == "multimodal" else None
    B = args.batch_size
    n_train = tr[0].shape[0]
    steps_per_epoch = n_train // B                                              # drop_last=True
    if steps_per_epoch < 1:
        raise SystemExit(f"batch size {B} exceeds the {n_train} training rows of this rank")

    torch.manual_seed(Config.RANDOM_SEED)
    model = make_model(kind, args.input_dim_a, args.input_dim_b, args.n_sites, args.latent_dim).to(dev).set_precision(args.precision)
    if world > 1:
        parallel.broadcast_parameters(model)
    optimizer = FusedAdamW(model.parameters(), lr=Config.LEARNING_RATE, weight_decay=Config.WEIGHT_DECAY)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=Config.LR_SCHEDULER_FACTOR,
                                                           patience=Config.LR_SCHEDULER_PATIENCE)
    run_id = datetime.now().strftime("%Y%m%d_%H%M%S")
    start_epoch, best_val, trigger = 0, float("inf"), 0
    if args.resume:
        extra = checkpoint.load_training_state(args.resume, model, optimizer, scheduler)
        start_epoch, best_val, trigger = int(extra.get("epoch", 0)), float(extra.get("best_val", float("inf"))), int(extra.get("trigger", 0))
        run_id = extra.get("run_id", run_id)
        if rank == 0:
            print(f"Resumed from {args.resume}: epoch {start_epoch}, best validation loss {best_val:.2f}")
    os.makedirs(args.checkpoint_dir, exist_ok=True)
    if rank == 0:
        print(f"Starting {KINDS[kind]['title']} training run: {run_id}  ({n_train} rows/rank x {world} rank(s), batch {B}, {args.precision}, {args.input_dtype} inputs)")

    graphed = None
    if args.eager:
        if world > 1:
            parallel.attach(model)
    else:
        reduce = (lambda flat, async_op=False: dist.all_reduce(flat, op=dist.ReduceOp.SUM, async_op=async_op)) if world > 1 else None
        beta0 = min(1.0, start_epoch / Config.BETA_WARMUP_EPOCHS) * Config.BETA_START
        graphed = GraphedTrainStep(model, optimizer, beta=beta0, gamma=Config.GAMMA, class_weights=class_weights, warmup=1,
                                   preserve_state=True, reduce=reduce, kind=kind, dataset=tuple(tr), batch_size=B)

    perm_gen = torch.Generator(device=dev).manual_seed(Config.RANDOM_SEED + 1000 * rank)
    for epoch in range(start_epoch, args.epochs):
        model.train()
        beta = min(1.0, epoch / Config.BETA_WARMUP_EPOCHS) * Config.BETA_START          # train_dna2rna.py:80
        perm_gen.manual_seed(Config.RANDOM_SEED + 1000 * rank + epoch)                  # the epoch's shuffle is a function of (seed, rank, epoch): resumable
        order = torch.randperm(n_train, device=dev, generator=perm_gen)
        t0, running, steps = time.time(), 0.0, 0
        if graphed is not None:
            graphed.set_beta(beta)
            for i in range(steps_per_epoch):
                graphed.set_indices(order[i * B:(i + 1) * B])
                prev = graphed.step_logged()
                if prev is not None:
                    running += prev[0]
            running += graphed.flush_logged()[0]
            graphed.reset_logged()                                                # next epoch starts a fresh logging pipeline
            steps = steps_per_epoch
        else:
            for i in range(steps_per_epoch):
                idx = order[i * B:(i + 1) * B]
                a, b, s = tr[0][idx], tr[1][idx], tr[2][idx]
                loss = forward_loss(kind, model, a, b, s, beta, class_weights)
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
                running += loss.item()
                steps += 1
        torch.cuda.synchronize()
        dt = time.time() - t0
        if world > 1:
            parallel.average_bn_buffers(model)                                    # same eval-mode model on every rank
        model.eval()
        val_loss, vsteps = 0.0, 0
        with torch.no_grad():
            for i in range(0, va[0].shape[0], B):
                a, b, s = va[0][i:i + B], va[1][i:i + B], va[2][i:i + B]
                val_loss += forward_loss(kind, model, a, b, s, beta, class_weights).item()
                vsteps += 1
        val_loss /= max(vsteps, 1)
        if world > 1:
            # eps is sampled in eval mode too (vae.py:73) and the Philox streams differ per rank: the scheduler / checkpoint /
            # early-stop decisions below must see ONE number on every rank or the ranks part ways
            val_loss = parallel.all_ranks_mean(val_loss, dev)
        scheduler.step(val_loss)                                                  # a new LR reaches the captured step through its device scalar
        if rank == 0:
            print(f"Epoch [{epoch + 1}/{args.epochs}] | Train Loss: {running / max(steps, 1):.2f} | Val Loss: {val_loss:.2f} | "
                  f"beta={beta:.5f} | lr={optimizer.param_groups[0]['lr']:.2e} | {world * steps * B / dt:,.0f} samples/s")
        if args.log_json:
            import json
            with open(f"{args.log_json}.rank{rank}", "a") as f:
                f.write(json.dumps(dict(epoch=epoch + 1, steps=steps, train_loss=running / max(steps, 1), val_loss=val_loss,
                                        lr=optimizer.param_groups[0]["lr"], best_val=min(best_val, val_loss), trigger=trigger)) + "\n")
        stop = False
        if val_loss < best_val:
            best_val, trigger = val_loss, 0
            if rank == 0:
                torch.save(model.state_dict(), os.path.join(args.checkpoint_dir, f"best_{tag}_{run_id}.pt"))
        else:
            trigger += 1
            stop = trigger >= Config.PATIENCE
        if args.save_state and rank == 0:
            checkpoint.save_training_state(args.save_state, model, optimizer, scheduler, epoch=epoch + 1, best_val=best_val,
                                           trigger=trigger, run_id=run_id)
        if stop:
            if rank == 0:
                print(f"Early stopping triggered at epoch {epoch + 1}!")
            break
    if rank == 0:
        with open(f"latest_{tag}_run_id.txt", "w") as f:                            # train_dna2rna.py:244-245
            f.write(run_id)
        print(f"Training complete. Run ID: {run_id}. Best validation loss: {best_val:.2f}")
    if world > 1:
        dist.destroy_process_group()
