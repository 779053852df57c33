"""What every driver does around its Engine: one process per GPU with a tcp://127.0.0.1 rendezvous (pretrain.py:263-336 of the
reference, framework/utils/distributed.py), logging with the run's experiment.log (framework/logging.py), seeding
(utils/reproduction.py), the config with its -x overlays, the checkpoint arch check and the per-epoch scalars line."""
import json
import logging
import os
import random
import socket
import sys
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

from .arguments import _merge, save_run_files


def setup_logging(args, local_rank: int):
    logging.basicConfig(level=logging.DEBUG if args.debug else logging.INFO, format="%(asctime)s %(message)s")
    if local_rank == 0 and args.run_dir is not None:
        Path(args.run_dir).mkdir(parents=True, exist_ok=True)
        logging.getLogger().addHandler(logging.FileHandler(Path(args.run_dir) / "experiment.log"))   # framework/logging.py:31


def seed_everything(seed):
    """utils/reproduction.py initialize_seed; None leaves the generators alone."""
    if seed is not None:
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)


def load_config(path, ext_config) -> dict:
    with open(path) as f:
        cfg = json.load(f)
    for snippet in ext_config or []:                                # -x overlays: JSON objects merged on top
        _merge(cfg, json.loads(snippet))
    return cfg


def save_run(args, cfg: dict, local_rank: int):
    """Rank 0 creates the experiment directory and writes the run's files."""
    if local_rank == 0:
        Path(args.experiment_dir).mkdir(parents=True, exist_ok=True)
        save_run_files(args, cfg)


def init_process_group(args, local_rank: int, dist_url: str, forced: bool = False) -> bool:
    """The NCCL group of a run with more than one rank -- or of one rank when ``forced``.  Returns whether there is one."""
    active = args.world_size > 1 or forced
    if active:
        dist.init_process_group("nccl", init_method=dist_url or f"tcp://127.0.0.1:{_free_port()}", rank=local_rank,
                                world_size=max(args.world_size, 1), device_id=torch.device("cuda", local_rank))
    return active


def finish_process_group(active: bool):
    if active:
        dist.barrier()
        dist.destroy_process_group()


def launch(main_worker, args):
    """main_worker(local_rank, args, dist_url): inline at one rank (its result is returned), else one spawned process per rank."""
    if args.world_size <= 1:
        return main_worker(0, args, "")
    torch.multiprocessing.spawn(main_worker, args=(args, f"tcp://127.0.0.1:{_free_port()}"), nprocs=args.world_size)


def load_states(path, device, arch: str) -> dict:
    """torch.load of a checkpoint dict, refused unless it is of architecture ``arch`` (pretrain.py:112-116)."""
    states = torch.load(path, map_location=device, weights_only=False)
    if states["arch"] != arch:
        raise ValueError(f'Loading checkpoint arch {states["arch"]} does not match current arch {arch}')
    return states


def append_scalars(path, record: dict):
    """One JSON line per epoch in RUN_DIR/scalars.jsonl: what the reference hands to its summary writer.  ``path`` None: nothing."""
    if path is not None:
        path.parent.mkdir(parents=True, exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def visible_gpu_count() -> int:
    """Number of GPUs a launcher spawns ranks for — what the reference asks torch.cuda.device_count() for (pretrain.py:318) —
    found WITHOUT touching the HIP runtime in the parent: ranks are fresh child processes and the launcher itself must stay
    GPU-free (a process that has initialised the GPU must never be re-exec'ed or forked on this platform).  A short-lived CHILD
    interpreter is asked for torch.cuda.device_count(): it sees exactly what a rank will see (HIP_/ROCR_/CUDA_VISIBLE_DEVICES,
    container device filtering).  Only if that child cannot be run, the count falls back to the KFD topology intersected with the
    *_VISIBLE_DEVICES lists.  Raises when no GPU is visible."""
    import subprocess
    n = None
    try:
        r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True,
                           timeout=300)
        if r.returncode == 0:
            n = int(r.stdout.strip().splitlines()[-1])
    except (OSError, ValueError, IndexError, subprocess.TimeoutExpired):
        n = None
    if n is None:
        n = _kfd_gpu_count()
        for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):      # each list filters the previous one
            v = os.environ.get(var)
            if v is not None:
                n = min(n, len([t for t in v.split(",") if t.strip() != ""]))
    if n <= 0:
        raise EnvironmentError("rspnet_amd.pretrain: no GPU is visible to this process (check HIP_VISIBLE_DEVICES / "
                               "ROCR_VISIBLE_DEVICES and the container's /dev/kfd, /dev/dri access); pass --ws to override")
    return n


def _kfd_gpu_count() -> int:
    """GPUs in the KFD topology (nodes with simd_count > 0)."""
    import glob
    n = 0
    for path in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
        try:
            with open(path) as f:
                props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
            if int(props.get("simd_count", "0")) > 0:
                n += 1
        except (OSError, ValueError):
            continue
    return n
