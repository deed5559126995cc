"""Training driver -- counterpart of the reference's train_flow.py:38-194 on the MI355X path: the same YAML keys,
the same loop (forward per input window, `event_flow_association`, loss / backward / clip / optimizer step once
`window_loss` events are collected, `detach_states`, `reset`), the models / loss of `event_flow_amd`.

Differences, all host side: MLflow and the visualiser are optional extras of the reference and not used here (metrics
go to stdout and `--out` receives the checkpoint).  Data: the sequence files under `data.path` (HDF5 through h5py, or
the `.npz` flavour of the same layout, event_flow_amd/dataloader/h5.py), or `--synthetic` windows (moving dots with
known motion).  `--fused-optimizer` swaps `clip_grad_norm_` + `torch.optim.Adam` for the fused flat-buffer kernel
(same update rule).  `--resident --graphed --fused-optimizer` replays every optimizer step from a hipGraph that begins at the
cut out of the device-resident sequences (event_flow_amd.train.ResidentWindowStep).  `vis.store_grads: True` (the reference's
key) or `--monitor DIR` log every optimizer step: `DIR/grads_w.csv` (mean, min, max of |grad| per weight tensor after clipping, the
reference's layout) and, with `--fused-optimizer`, `DIR/train_log.csv` (loss, gradient norm, clip coefficient, spike rate per
layer), collected on the device without a host read per step (event_flow_amd.monitor.TrainMonitor).

  python train_flow.py --config configs/train_SNN.yml --synthetic [--epochs 5] [--out model.pth]
"""

import argparse
import json
import os
import time

import torch

from event_flow_amd.configs.parser import YAMLParser
from event_flow_amd.loss.flow import EventWarping
from event_flow_amd.models.model import MODELS
from event_flow_amd import monitor as monitoring
from event_flow_amd.parallel import DataParallel
from event_flow_amd.train import FlatAdam
from event_flow_amd.utils.utils import load_model


def _graphed_refusal(args):
    """Why --graphed cannot serve this call (None: it can), from the arguments and the environment alone."""
    if args.synthetic:
        return "--graphed replays windows cut out of device-resident sequence files; --synthetic has none"
    if not getattr(args, "resident", False):
        return "--graphed needs --resident: the replayed step begins at the cut out of the sequences in device memory"
    if not args.fused_optimizer:
        return "--graphed needs --fused-optimizer: the replayed step ends in the flat clip + Adam kernel"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return ("--graphed runs on one rank: the ranks would have to agree on every batch's restart flag while the windows are "
                "planned; use --resident without --graphed under torch.distributed.run")
    return None


MONITOR_ROWS = 1024  # rows of the monitor's device log: drained at every epoch end and whenever the ring is about to wrap


def _monitor_dir(args, config):
    """Where the step logs go (None: no monitor): --monitor DIR, or with vis.store_grads the directory of --out, or "."."""
    directory = getattr(args, "monitor", None)
    if directory is None and config["vis"].get("store_grads", False):
        directory = os.path.dirname(args.out) if args.out else "."
    return (directory or ".") if directory is not None else None


def train_graphed(args, config, model, loss_function, optimizer, data, n_epochs, replay=True, monitor=None, csvlog=None):
    """The epochs of `train` with every optimizer step taken by a ResidentWindowStep: the same steps on the same batches as the
    loop below (ResidentPlan.plan_steps), per-epoch losses and the best-loss checkpoint by the same arithmetic, closed when the
    first step of a later epoch arrives and after the last step.  -> (history, best loss, the stepper's counters)."""
    from event_flow_amd.train import ResidentWindowStep

    P = -(-int(config["data"]["window_loss"]) // int(config["data"]["window"]))  # passes until window_loss events are collected
    stepper = ResidentWindowStep(model, loss_function, optimizer, data, P, replay=replay, monitor=monitor)
    device = data.device
    best_loss, history = 1.0e6, []
    t_start = time.time()
    state = {"loss": torch.zeros((), device=device), "samples": 0, "steps": 0}

    def close_epoch():
        nonlocal best_loss
        epoch_loss = float(state["loss"]) / max(state["samples"], 1)
        if monitor is not None:  # (the epoch end synchronises already)
            csvlog.write(len(history), monitor.drain())
        history.append(epoch_loss)
        if config["vis"].get("verbose", False):
            print("Train Epoch: {:04d}  Loss: {:.6f}  ({} optimizer steps, {:.1f} s)".format(len(history) - 1, epoch_loss,
                                                                                             state["steps"], time.time() - t_start))
        if epoch_loss < best_loss:
            best_loss = epoch_loss
            if args.out:
                torch.save(model.state_dict(), args.out)
        state.update(loss=torch.zeros((), device=device), samples=0, steps=0)

    for discarded, group, reset, epoch in data.plan_steps(P, n_epochs):
        while len(history) < epoch:
            close_epoch()
        if monitor is not None and monitor.full:  # the ring is about to wrap
            csvlog.write(len(history), monitor.drain())
        loss, _info = stepper.step((discarded, group, reset))
        with torch.cuda.stream(stepper.stream):  # before the next replay rewrites the graph's loss tensor
            state["loss"] += loss
        torch.cuda.current_stream().wait_stream(stepper.stream)
        state["samples"] += config["loader"]["batch_size"]
        state["steps"] += 1
    while len(history) < n_epochs:
        close_epoch()
    return history, best_loss, dict(stepper.stats)


def train(args, config_parser, graphed_replay=True):
    """`graphed_replay=False`: with --graphed, every step runs the window's launches eagerly (the A/B of the replay)."""
    graphed = getattr(args, "graphed", False)
    if graphed and _graphed_refusal(args):
        raise SystemExit(_graphed_refusal(args))
    config = config_parser.config
    if config["data"]["mode"] == "frames":
        print("Config error: Training pipeline not compatible with frames mode.")
        raise AttributeError
    config = config_parser.combine_entries(config)
    monitor_dir = _monitor_dir(args, config)
    if monitor_dir is not None:  # (refused on the host, before any device work)
        why = monitoring.refusal(fused_optimizer=bool(args.fused_optimizer), want_rates=getattr(args, "monitor", None) is not None)
        if why:
            raise SystemExit(why)
    model = None
    if graphed:  # (built on the host first: the refusal comes before any device work)
        model = MODELS[config["model"]["name"]](config["model"].copy())
        path, why = getattr(model, "compute_path", ("general", "no FireNet-family network"))
        if path != "fused":
            raise SystemExit(f"--graphed replays the fused FireNet engine's step; {config['model']['name']} runs on the general "
                             f"path ({why}): use --resident without --graphed")
    device = config_parser.device
    if torch.device(device).type == "cuda":
        torch.cuda.set_device(device)  # the evf_* launches go to the current device's stream (loader.gpu may not be 0)

    # data parallel (one process per GPU under torch.distributed.run): sequence files sharded over the ranks, one SUM
    # all-reduce of the flat gradient per optimizer step (event_flow_amd/parallel.py)
    dp = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        if not args.fused_optimizer:
            raise SystemExit("data-parallel training reduces the flat gradient buffer: add --fused-optimizer")
        if not os.environ.get("EVF_BENCH_SINGLE_DEVICE"):  # (test hook: all ranks on the one GPU of the box)
            device = torch.device(f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}")
            torch.cuda.set_device(device)
        dp = DataParallel(device=device)
    rank, world = (dp.rank, dp.world) if dp else (0, 1)

    if args.synthetic:
        from event_flow_amd.dataloader.synthetic_loader import SyntheticLoader

        data = SyntheticLoader(config, config["model"]["num_bins"], config["model"].get("round_encoding", False), device=device,
                               seed_offset=1000 * rank)
    elif getattr(args, "resident", False):  # the sequence files uploaded once, every batch cut and filtered on the GPU
        from event_flow_amd.dataloader.resident import ResidentLoader

        data = ResidentLoader(config, config["model"]["num_bins"], config["model"].get("round_encoding", False), device=device,
                              rank=rank, world_size=world)
    else:
        from event_flow_amd.dataloader.h5 import H5Loader

        data = H5Loader(config, config["model"]["num_bins"], config["model"].get("round_encoding", False), device=device,
                        rank=rank, world_size=world)

    loss_function = EventWarping(config, device)
    model = (model if model is not None else MODELS[config["model"]["name"]](config["model"].copy())).to(device)
    if args.prev:  # a state_dict file, a reference checkpoint (pickled model) or its MLflow run id under ./mlruns
        model = load_model(args.prev, model, device)
    model.train()

    clip = config["loss"].get("clip_grad", None)
    if args.fused_optimizer:
        optimizer = FlatAdam(model, lr=config["optimizer"]["lr"], clip=clip, device_step=graphed)
    else:
        optimizer = getattr(torch.optim, config["optimizer"]["name"])(model.parameters(), lr=config["optimizer"]["lr"])
    if dp:  # every rank starts from rank 0's parameters
        dp.broadcast(optimizer.flat_param)
        optimizer.step_invalidate()
    optimizer.zero_grad()
    monitor = csvlog = None
    if monitor_dir is not None and args.fused_optimizer:
        monitor = monitoring.TrainMonitor(model, optimizer, rows=MONITOR_ROWS)
        csvlog = monitoring.CsvLog(monitor_dir, monitor.columns())
    elif monitor_dir is not None:  # vis.store_grads beside torch's optimizer: read on the host after clip_grad_norm_
        from event_flow_amd.utils.gradients import get_grads

        csvlog = monitoring.CsvLog(monitor_dir, monitoring.grad_columns(model))

    n_epochs = args.epochs if args.epochs is not None else config["loader"]["n_epochs"]
    best_loss, history = 1.0e6, []
    t_start = time.time()
    data.shuffle()  # once, before the first epoch (train_flow.py:92)
    if graphed:
        history, best_loss, counters = train_graphed(args, config, model, loss_function, optimizer, data, n_epochs, graphed_replay,
                                                     monitor, csvlog)
        print(json.dumps({"model": config["model"]["name"], "epochs": n_epochs, "loss_per_epoch": history, "best_loss": best_loss,
                          "ranks": world, "graphed": counters}))
        return history
    for epoch in range(n_epochs):
        train_loss, samples, steps = torch.zeros((), device=device), 0, 0
        host_grads = []  # vis.store_grads without the fused optimizer: one get_grads dict per step
        batches = iter(data)
        while True:
            inputs = next(batches, None)
            new_seq, done = bool(inputs is not None and data.new_seq), inputs is None
            if dp:  # the ranks reset and end their epochs together
                new_seq, done = dp.any_flags([new_seq, done])
            if done:
                break
            if new_seq:  # any slot restarted: reset everything (train_flow.py:100-105)
                data.new_seq = False
                loss_function.reset()
                model.reset_states()
                optimizer.zero_grad()
                if monitor is not None:
                    monitor.begin_window()  # (the spike words of the passes dropped here)

            x = model(inputs["event_voxel"], inputs["event_cnt"])
            loss_function.event_flow_association(x["flow"], inputs["event_list"], inputs["event_list_pol_mask"],
                                                 inputs["event_mask"])

            # The optimizer step contains the step's collective, so with several ranks the decision to step is itself
            # made collectively: `num_events` is a rank-local count (it differs between ranks in the time / gtflow
            # modes), and a rank entering the all-reduce alone would pair it with another rank's flag exchange.
            step_now = loss_function.num_events >= config["data"]["window_loss"]
            if dp:
                step_now = dp.any_flags([step_now])[0]
            if step_now:
                if config["loss"]["overwrite_intermediate"]:
                    loss_function.overwrite_intermediate_flow(x["flow"])
                loss = loss_function()
                samples += config["loader"]["batch_size"] * world
                steps += 1
                if monitor is not None:
                    if monitor.full:  # the ring is about to wrap
                        csvlog.write(epoch, monitor.drain())
                    monitor.count_spikes()
                loss.backward()
                if dp:  # gradient (+ loss) summed over the ranks: the step below is the global-batch step
                    loss = dp.all_reduce_grads(optimizer.comm, loss)[0]
                train_loss += loss.detach()  # no host sync inside the loop
                if args.fused_optimizer:
                    if monitor is not None:
                        monitor.before_step()  # (the step clears the gradient)
                    optimizer.step()  # clip + Adam in one kernel
                    if monitor is not None:
                        monitor.after_step(loss)
                else:
                    if clip is not None:
                        torch.nn.utils.clip_grad.clip_grad_norm_(model.parameters(), clip)
                    if csvlog is not None:
                        host_grads.append(get_grads(model.named_parameters()))
                    optimizer.step()
                optimizer.zero_grad()
                model.detach_states()
                loss_function.reset()
        if hasattr(batches, "close"):
            batches.close()  # a rank that stops early (another rank ran out of files) ends its reader thread here
        epoch_loss = float(train_loss) / max(samples, 1)
        history.append(epoch_loss)
        if monitor is not None:  # (the epoch end synchronises already)
            csvlog.write(epoch, monitor.drain())
        elif csvlog is not None and host_grads:
            csvlog.write(epoch, [[g[c] for c in csvlog.grad_header[1:]] for g in host_grads])
        if config["vis"].get("verbose", False) and rank == 0:
            print("Train Epoch: {:04d}  Loss: {:.6f}  ({} optimizer steps, {:.1f} s)".format(epoch, epoch_loss, steps,
                                                                                             time.time() - t_start))
        if epoch_loss < best_loss:
            best_loss = epoch_loss
            if args.out and rank == 0:
                torch.save(model.state_dict(), args.out)
    if dp:
        dp.barrier()
        dp.close()
    if rank == 0:
        print(json.dumps({"model": config["model"]["name"], "epochs": n_epochs, "loss_per_epoch": history, "best_loss": best_loss,
                          "ranks": world}))
    return history


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", default="configs/train_SNN.yml", help="training configuration")
    parser.add_argument("--synthetic", action="store_true", help="synthetic moving-dots windows instead of HDF5 files")
    parser.add_argument("--prev", default="", help="state_dict to resume from (reference: --prev_runid)")
    parser.add_argument("--out", default="", help="where to save the best state_dict")
    parser.add_argument("--epochs", type=int, default=None)
    parser.add_argument("--fused-optimizer", action="store_true")
    parser.add_argument("--resident", action="store_true",
                        help="keep the sequence files in device memory and cut the input windows there (data.mode events)")
    parser.add_argument("--graphed", action="store_true",
                        help="with --resident --fused-optimizer: replay every optimizer step, from the cut to clip + Adam, from a hipGraph")
    parser.add_argument("--monitor", default=None, metavar="DIR",
                        help="log every optimizer step to DIR/grads_w.csv and DIR/train_log.csv (with --fused-optimizer: gradient "
                             "statistics and spike rates collected on the device)")
    args = parser.parse_args()
    train(args, YAMLParser(args.config))
