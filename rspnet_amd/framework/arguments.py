"""The command line the drivers share (arguments.py, framework/arguments.py of the reference: flag names, run directories,
--continue) and the files a run leaves in its directory."""
import json
import logging
import os
import re
import sys
from datetime import datetime
from pathlib import Path
from shlex import quote

logger = logging.getLogger(__name__)
RUN_DIR_NAME_REGEX = re.compile(r"^run_(\d+)_")


def add_driver_arguments(ap, config_example: str, world_size):
    """The flags of both training drivers.  ``world_size``: the default of --ws (None: the driver counts the visible GPUs)."""
    ap.add_argument("-c", "--config", default=None, help=f"resolved config JSON (e.g. {config_example})")
    ap.add_argument("-x", "--ext-config", action="append", help="JSON object merged over the config (may repeat)")
    ap.add_argument("-e", "--experiment-dir", required=True)
    ap.add_argument("--load-checkpoint", default=None, help="a checkpoint of this driver: model, optimizer, scheduler, epoch")
    ap.add_argument("-d", "--debug", action="store_true", help="1 epoch, DEBUG logging")
    ap.add_argument("--ws", "--world-size", dest="world_size", type=int, default=world_size)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--run-dir", default=None, help="default: EXP/run_{id}_{timestamp}")
    ap.add_argument("--continue", dest="cont", action="store_true", help="use the previous run's config and EXP/checkpoint.pth.tar")
    ap.add_argument("--steps-per-epoch", type=int, default=100, help="synthetic train loader length")


def parse_driver_args(ap, argv=None):
    """ap.parse_args, then --continue, the config requirement and the run directory, resolved once, before workers are spawned."""
    args = ap.parse_args(argv)
    resolve_continue(args)
    if args.config is None:
        ap.error("-c/--config is required (or --continue with a previous run)")
    args.run_dir = str(resolve_run_dir(args))
    return args


def resolve_run_dir(args) -> Path:
    """EXP/run_{id}_{timestamp}: id = 1 + the highest existing run id (framework/arguments.py:64-78)."""
    if args.run_dir is not None:
        return Path(args.run_dir)
    exp = Path(args.experiment_dir)
    run_id = -1
    if exp.exists():
        for prev in exp.iterdir():
            m = RUN_DIR_NAME_REGEX.match(prev.name)
            if m is not None:
                run_id = max(run_id, int(m.group(1)))
    return exp / f"run_{run_id + 1}_{datetime.now().strftime('%Y%m%d_%H%M%S')}"


def resolve_continue(args):
    """--continue: newest run's config.json and EXP/checkpoint.pth.tar (arguments.py:59-86)."""
    if not args.cont:
        return
    exp = Path(args.experiment_dir)
    if not exp.exists():
        raise EnvironmentError(f'Experiment directory "{exp}" does not exists.')
    if args.config is None:
        best = -1
        for run in exp.iterdir():
            m = RUN_DIR_NAME_REGEX.match(run.name)
            if m is not None and int(m.group(1)) > best and run.is_dir() and (run / "config.json").exists():
                best = int(m.group(1))
                args.config = str(run / "config.json")
        if args.config is None:
            raise EnvironmentError("No previous run config found")
        logger.info('Continue using previous config: "%s"', args.config)
    if args.load_checkpoint is None:
        ckpt = exp / "checkpoint.pth.tar"
        if ckpt.exists():
            args.load_checkpoint = str(ckpt)
            logger.info('Continue using previous checkpoint: "%s"', ckpt)
        else:
            logger.warning("No previous checkpoint found")


def save_run_files(args, cfg: dict):
    """run dir contents: config.json (framework/config.py:78-81), run.sh (framework/arguments.py:49-58), experiment.log."""
    run_dir = Path(args.run_dir)
    run_dir.mkdir(parents=True, exist_ok=True)
    with open(run_dir / "config.json", "w") as f:
        json.dump(cfg, f, indent=2)
    with open(run_dir / "run.sh", "w") as f:
        f.write(f"cd {quote(os.getcwd())}\n")
        for env in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
            if os.environ.get(env) is not None:
                f.write(f"export {env}={quote(os.environ[env])}\n")
        f.write(sys.executable + " " + " ".join(quote(a) for a in sys.argv) + "\n")


def _merge(base: dict, over: dict):
    for k, v in over.items():
        if isinstance(v, dict) and isinstance(base.get(k), dict):
            _merge(base[k], v)
        else:
            base[k] = v
