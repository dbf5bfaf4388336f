#!/usr/bin/env python
"""Data-parallel training driver with the loop semantics of the reference's train.py, on RCCL instead of
Horovod/MPI (one process per GPU: `python -m torch.distributed.run --nproc-per-node N train_dp.py`).

Kept from the reference (train.py:41-259): CLI flags -m/--model, --eval, --resume, --weight; seed = rank
(:55-59); the model plugin call import_module(model).get_model() (:63-64); parameter broadcast from rank 0
(:96,145); per-rank sampler shard with drop_last (:119-131); step order net -> loss -> post_process -> zero_grad ->
backward -> [gradient average] -> opt.step(epoch) with epoch += 1/num_batches per iteration (:175-186); checkpoint
dict {"epoch", "state_dict" (CPU tensors), "opt_state"} named "%3.3f.ckpt" (:230-242) every save_iters; display +
metrics reset every display_iters; a validation pass every val_iters and at the end (:189-208).  The gradient average
is ONE flat all-reduce (lanegcn_amd.dist.allreduce_mean_grads).  Difference: the sampler drops the shard's tail
where the reference's DistributedSampler pads it.

The reference's test.py (:60-100) is `--eval --eval-store PATH`: the whole store, every scene once over all ranks, through
lanegcn_amd.evaluate (Argoverse's forecasting metrics for K = num_mods and K = 1; `--save-preds` writes the predictions);
`--eval-actors [--min-obs N]` scores every actor with an observed future step and prints all / agent / others.
"""
import argparse
import os
import sys
import time
from importlib import import_module

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import lanegcn_amd  # noqa: E402,F401
from lanegcn_amd import dist as D  # noqa: E402
from lanegcn_amd.utils import load_pretrain  # noqa: E402


def save_ckpt(net, opt, save_dir, epoch):
    os.makedirs(save_dir, exist_ok=True)
    state = {k: v.cpu() for k, v in net.state_dict().items()}
    path = os.path.join(save_dir, "%3.3f.ckpt" % epoch)
    torch.save({"epoch": epoch, "state_dict": state, "opt_state": opt.opt.state_dict()}, path)
    return path


def batches(dataset, collate_fn, batch_size, rank, world, seed, epoch, shuffle=True):
    idx = D.shard(len(dataset), rank, world, seed=seed, epoch=epoch, shuffle=shuffle, drop_last=True)
    for i in range(0, len(idx) - batch_size + 1, batch_size):        # drop_last on the batch level too
        yield collate_fn([dataset[j] for j in idx[i:i + batch_size]])


def store_picks(n_scenes, batch_size, rank, world, seed, epoch):
    """The scene indices of every batch of `batches` (the same D.shard schedule), for a resident store of n_scenes."""
    idx = D.shard(n_scenes, rank, world, seed=seed, epoch=epoch, shuffle=True, drop_last=True)
    for i in range(0, len(idx) - batch_size + 1, batch_size):
        yield idx[i:i + batch_size]


def first_rows_on_host(data):
    """What PostProcess reads of a store batch: the first actor row per scene of gt_preds / has_preds (device views), each
    copied to the host once per step -> per-scene lists of host tensors (an empty one for a scene without actors)."""
    counts = [min(len(x), 1) for x in data["gt_preds"]]
    gt = torch.cat([x[0:1] for x in data["gt_preds"]]).cpu()
    has = torch.cat([x[0:1] for x in data["has_preds"]]).cpu()
    return {"gt_preds": list(torch.split(gt, counts)), "has_preds": list(torch.split(has, counts))}


def store_eval_picks(n_scenes, rank, world):
    """This rank's scenes of a store under evaluation: r, r + world, ... -- every scene once, no tail dropped."""
    return np.arange(rank, n_scenes, world, dtype=np.int64)


def metric_lines(summary, ks):
    """One line per K of an Evaluator.summary(), the metrics in Argoverse's key order."""
    return ["K=%d " % k + ", ".join("%s %.4f" % (m, v) for m, v in summary[k].items()) for k in ks]


def main(argv=None):
    ap = argparse.ArgumentParser(description="LaneGCN training on MI355X (RCCL data parallel)")
    ap.add_argument("-m", "--model", default="lanegcn_mi355x", type=str, metavar="MODEL", help="model plugin module")
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--resume", default="", type=str, metavar="RESUME", help="checkpoint path")
    ap.add_argument("--weight", default="", type=str, metavar="WEIGHT", help="checkpoint path (weights only)")
    ap.add_argument("--max-iters", type=int, default=0, help="stop after this many iterations (smoke runs)")
    ap.add_argument("--batch-size", type=int, default=0, help="override config['batch_size']")
    ap.add_argument("--save-dir", default="", help="override config['save_dir']")
    ap.add_argument("--dataset-len", type=int, default=0, help="synthetic dataset length override")
    ap.add_argument("--store", default="", type=str, metavar="PATH",
                    help="train from this flat store (flatfile.write_scenes), resident on the device; validation keeps the dataset "
                         "unless --eval-store is given")
    ap.add_argument("--eval-store", default="", type=str, metavar="PATH",
                    help="a flat store with gt_preds (the validation split), resident on the device: with --eval the whole store "
                         "is evaluated (Argoverse's forecasting metrics for K = num_mods and K = 1); without it, validation "
                         "runs from this store instead of the dataset")
    ap.add_argument("--eval-replay", action="store_true",
                    help="with --eval --eval-store: pad every full batch to fixed sizes and replay one captured graph "
                         "(evaluate_store(..., replay=True)); same records")
    ap.add_argument("--save-preds", default="", type=str, metavar="FILE.npz",
                    help="with --eval --eval-store: write index, preds [n, num_mods, num_preds, 2] and scores [n, num_mods]")
    ap.add_argument("--eval-actors", action="store_true",
                    help="with --eval --eval-store: score every actor with an observed future step, not the agents alone; prints "
                         "the summaries of all actors, the agents and the others; --save-preds then also writes scene and local "
                         "and holds every actor")
    ap.add_argument("--min-obs", type=int, default=1, metavar="N",
                    help="with --eval-actors: an actor counts only with at least N observed future steps")
    ap.add_argument("--eval-drivable", default="", type=str, metavar="FILE.npz",
                    help="with --eval --eval-store: also print DAC (drivable-area compliance) per K.  The file holds cities "
                         "[C] (names), raster/<city> and se2/<city> (Argoverse's two arrays per city) and scene_city [S] int32 "
                         "(the city id of every scene of the store, -1: no map); INTEGRATION.md shows how to write it")
    ap.add_argument("--rot-size", type=float, default=None, metavar="X",
                    help="turn every picked scene by rand() * X per step (needs a store written with theta=True); default: "
                         "config['rot_size'] when config['rot_aug'] is set, else no augmentation")
    args = ap.parse_args(argv)

    rank, world, local_rank = D.env_ranks()
    torch.cuda.set_device(local_rank)
    if world > 1:
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    seed = rank                                                   # train.py:55-59
    torch.manual_seed(seed)
    np.random.seed(seed)

    model = import_module(args.model)
    config, Dataset, collate_fn, net, loss, post_process, opt = model.get_model()
    if args.batch_size:
        config["batch_size"] = args.batch_size
    if args.save_dir:
        config["save_dir"] = args.save_dir
    if args.resume or args.weight:
        ckpt = torch.load(args.resume or args.weight, map_location="cpu", weights_only=True)
        load_pretrain(net, ckpt["state_dict"])
        if args.resume:
            config["epoch"] = ckpt["epoch"]
            opt.load_state_dict(ckpt["opt_state"])
        if rank == 0 and (args.weight or args.eval):               # loaded weights run inference in the default f16x2 mode
            from tools.check_weight_scale import warn_small_blocks
            warn_small_blocks(ckpt["state_dict"])
    D.broadcast_parameters(net.state_dict().values(), 0)

    kw = {"length": args.dataset_len} if args.dataset_len else {}
    dataset = Dataset(config.get("train_split"), config, train=True, **kw)
    store, rot_size = None, None
    if args.store and not args.eval:
        from lanegcn_amd.flatfile import DeviceSceneStore, draw_rot_dt
        store = DeviceSceneStore(args.store)
        if args.rot_size is not None:
            rot_size = args.rot_size
        elif config.get("rot_aug"):
            rot_size = config["rot_size"]
    ks = sorted({config["num_mods"], 1}, reverse=True)
    if args.eval and args.eval_store:                              # the reference's test.py: the whole split, every scene once
        from lanegcn_amd.evaluate import Evaluator, evaluate_store
        from lanegcn_amd.flatfile import DeviceSceneStore
        eval_store = DeviceSceneStore(args.eval_store)
        da = {}
        if args.eval_drivable:
            from lanegcn_amd.evaluate import DrivableArea
            with np.load(args.eval_drivable) as z:
                cities = [str(c) for c in z["cities"]]
                da = dict(drivable=DrivableArea({c: (z["raster/" + c], z["se2/" + c]) for c in cities}),
                          scene_city=z["scene_city"].astype(np.int32))
        if args.eval_actors:
            from lanegcn_amd.evaluate import ActorEvaluator
            ev = ActorEvaluator.for_store(eval_store, config, keep_preds=bool(args.save_preds), **da)
        else:
            ev = Evaluator(len(eval_store), config["num_mods"], config["num_preds"], keep_preds=bool(args.save_preds), **da)
        net.eval()
        evaluate_store(net, eval_store, config["val_batch_size"], ev, indices=store_eval_picks(len(eval_store), rank, world),
                       replay=args.eval_replay)
        ev.merge()
        if args.eval_actors:
            for who in ("all", "agent", "others"):
                summary = ev.summary(ks=ks, who=who, min_obs=args.min_obs)
                if rank == 0:
                    print("actors: %s, at least %d observed steps" % (who, args.min_obs))
                    print("\n".join(metric_lines(summary, ks)))
                    print("evaluated %d actors, skipped %d, non-finite %d, excluded %d"
                          % (summary["n_evaluated"], summary["n_skipped"], summary["n_nonfinite"], summary["n_excluded"]))
            if rank == 0 and args.save_preds:
                index, preds, scores = ev.predictions()
                scene, local = ev.actor_index()
                np.savez(args.save_preds, index=index, scene=scene[index], local=local[index], preds=preds, scores=scores)
            if world > 1:
                torch.distributed.destroy_process_group()
            return 0
        summary = ev.summary(ks=ks)
        if rank == 0:
            print("\n".join(metric_lines(summary, ks)))
            print("evaluated %d scenes, skipped %d, non-finite %d"
                  % (summary["n_evaluated"], summary["n_skipped"], summary["n_nonfinite"]))
            if args.save_preds:
                index, preds, scores = ev.predictions()
                np.savez(args.save_preds, index=index, preds=preds, scores=scores)
        if world > 1:
            torch.distributed.destroy_process_group()
        return 0
    if args.eval:
        net.eval()
        with torch.no_grad():
            for data in batches(dataset, collate_fn, config["val_batch_size"], rank, world, 0, 0, shuffle=False):
                out = net(data)
                loss_out = loss(out, data)
                if rank == 0:
                    print("val loss %.4f" % float(loss_out["loss"]))
                break
        return 0

    # The reference runs its training loop on one Python thread per GPU (train.py:8-10, 175-186); with ~375 Python
    # autograd Functions in a backward, running them on the calling thread instead of the engine's device thread
    # saves 12 % of a step.  Scoped to this driver (LGCN_AUTOGRAD_MT=1 keeps torch's default).
    if os.environ.get("LGCN_AUTOGRAD_MT", "0") != "1":
        torch.autograd.set_multithreading_enabled(False)
    val_set = Dataset(config.get("val_split"), config, train=False, **kw)

    eval_store = None
    if args.eval_store:
        from lanegcn_amd.evaluate import Evaluator, evaluate_store
        from lanegcn_amd.flatfile import DeviceSceneStore
        eval_store = DeviceSceneStore(args.eval_store)

    def validate_store(epoch):
        """validate() from the resident store: ADE / FDE from the evaluator's records (K = 1 and K = num_mods), the loss
        from loss(out, data) per batch on the store's gt_preds / has_preds; the reference's validation line."""
        net.eval()
        t_val, vm = time.time(), dict()
        ev = Evaluator(len(eval_store), config["num_mods"], config["num_preds"])

        def batch_loss(out, fb, ex):
            data = {"gt_preds": [ex["gt_preds"]], "has_preds": [ex["has_preds"]]}
            post_process.append(vm, loss({"cls": [out["cls"]], "reg": [out["reg"]]}, data), {})

        evaluate_store(net, eval_store, config["val_batch_size"], ev, indices=store_eval_picks(len(eval_store), rank, world),
                       on_batch=batch_loss)
        ev.merge()
        summary = ev.summary(ks=ks)
        vm = D.gather_metrics(vm)
        if rank == 0 and vm:
            print("************************* Validation, time %3.2f *************************" % (time.time() - t_val))
            cls = vm["cls_loss"] / (vm["num_cls"] + 1e-10)
            reg = vm["reg_loss"] / (vm["num_reg"] + 1e-10)
            print("loss %2.4f %2.4f %2.4f, ade1 %2.4f, fde1 %2.4f, ade %2.4f, fde %2.4f"
                  % (cls + reg, cls, reg, summary[1]["minADE"], summary[1]["minFDE"], summary[ks[0]]["minADE"],
                     summary[ks[0]]["minFDE"]))
            print()
        net.train()

    def validate(epoch):                                             # train.py:200-216
        if eval_store is not None:
            return validate_store(epoch)
        net.eval()
        t_val, vm = time.time(), dict()
        with torch.no_grad():
            for vdata in batches(val_set, collate_fn, config["val_batch_size"], rank, world, 0, 0, shuffle=False):
                vout = net(vdata)
                post_process.append(vm, loss(vout, vdata), post_process(vout, vdata))
        vm = D.gather_metrics(vm)
        if rank == 0 and vm:
            post_process.display(vm, time.time() - t_val, epoch)
        net.train()

    net.train()
    # The shard drops the tail that does not divide by the world size and by the batch size (the reference's
    # DistributedSampler pads the shard by repeating samples, train.py:119-131; its DataLoader then drops the last
    # partial batch): every rank sees the same number of full batches either way.
    per_rank = len(store if store is not None else dataset) // world
    num_batches = max(per_rank // config["batch_size"], 1)
    save_iters = int(np.ceil(config["save_freq"] * num_batches))                       # train.py:166-171
    display_iters = max(int(config["display_iters"] / (world * config["batch_size"])), 1)
    val_iters = max(int(config["val_iters"] / (world * config["batch_size"])), 1)
    # a resumed epoch is a float accumulated in steps of 1 / num_batches: snap it to the batch grid before int()
    epoch = round(float(config["epoch"]) * num_batches) / num_batches
    it, t0, metrics = 0, time.time(), dict()
    last_path, done = None, False
    bucket = D.GradBucket(net.parameters())                        # persistent flat gradient buffer (p.grad = views of it)
    for ep in range(int(epoch + 0.5 / num_batches), config["num_epochs"]):
        if store is not None:
            feed = store_picks(len(store), config["batch_size"], rank, world, seed=0, epoch=ep)
        else:
            feed = batches(dataset, collate_fn, config["batch_size"], rank, world, seed=0, epoch=ep)
        for data in feed:
            epoch += 1.0 / num_batches
            if store is not None:                                  # `data` is the pick: one launch cuts (and turns) the batch
                rot_dt = None if rot_size is None else draw_rot_dt(len(data), rot_size)
                out, data = net.forward_store_train(store, data, rot_dt=rot_dt)
                loss_out = loss(out, data)
                post_out = post_process(out, first_rows_on_host(data))
            else:
                out = net(data)
                loss_out = loss(out, data)
                post_out = post_process(out, data)
            post_process.append(metrics, loss_out, post_out)
            bucket.zero()                                          # the reference's opt.zero_grad(): one fill of the flat bucket
            loss_out["loss"].backward()                            # accumulates into the bucket's views
            bucket.allreduce_mean()                                # Horovod DistributedOptimizer semantics, one in-place all-reduce
            lr = opt.step(epoch)
            it += 1
            num_iters = int(np.round(epoch * num_batches))
            finished = epoch >= config["num_epochs"] or (args.max_iters and it >= args.max_iters)
            if rank == 0 and (num_iters % save_iters == 0 or finished):                 # train.py:189-193
                last_path = save_ckpt(net, opt, config["save_dir"], epoch)
            if num_iters % display_iters == 0 or (args.max_iters and it % 10 == 0):      # train.py:195-201
                metrics = D.gather_metrics(metrics)
                if rank == 0:
                    post_process.display(metrics, time.time() - t0, epoch, lr)
                t0, metrics = time.time(), dict()
            if num_iters % val_iters == 0 or finished:                                   # train.py:203-208
                validate(epoch)
            if finished:
                done = True
                break
        if done:
            break
    D.barrier()
    if rank == 0 and last_path:
        print("saved", last_path)
    if world > 1:
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
