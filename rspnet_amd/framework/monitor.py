"""The base of the pretext driver's opt-in epoch-end monitors (kNN, representation statistics, linear probe, clustering, t-SNE): what
they share -- the config block, the schedule, the argument checks, the capture refusal -- and the interface the driver's one loop
drives (``pretrain.Engine._run_monitors``).  This module imports none of the monitors; they import it.

A monitor is a subclass with ``KEY`` (its config key), ``KEYS`` (the keys its block accepts: the keyword arguments of its constructor
besides ``num_epochs``), a constructor that sets ``every`` and ``num_epochs``, ``run(model, *loaders) -> dict``, ``scalars`` and
``log_line``; ``build_loaders`` where it needs data.  Appending the class to ``pretrain.MONITORS`` is all the driver needs.
"""
from __future__ import annotations

from typing import Optional

import torch


class EpochMonitor:
    KEY = ""       # the config key, e.g. "knn_monitor"
    KEYS = ()      # the keys the config block accepts

    @classmethod
    def from_config(cls, cfg, num_epochs: int) -> Optional["EpochMonitor"]:
        """The ``KEY`` block of a pretext config, e.g. {"every": 10, ...}; None -- nothing constructed, no launch ever added -- when
        the key is absent, the block is empty or ``every`` is 0."""
        node = cfg.get(cls.KEY) if hasattr(cfg, "get") else None
        if not node or int(node.get("every", 0)) <= 0:
            return None
        extra = sorted(set(node) - set(cls.KEYS))
        if extra:
            raise ValueError(f"{cls.KEY}: unknown keys {extra}")
        return cls(num_epochs=num_epochs, **{key: node[key] for key in cls.KEYS if key in node})

    def due(self, epoch: int) -> bool:
        """``epoch``: the 0-based epoch that has just finished its last step."""
        return (int(epoch) + 1) % self.every == 0 or int(epoch) + 1 == self.num_epochs

    # ---- the checks of the constructors and of run ------------------------------------------------------------------------
    @classmethod
    def _check_encoder(cls, encoder):
        if encoder not in ("q", "k"):
            raise ValueError(f"{cls.KEY}: encoder must be 'q' or 'k', got {encoder!r}")

    @classmethod
    def _check_at_least_1(cls, **values):
        """ValueError unless every named value is an integer >= 1; the message lists the names in the order given."""
        if min(int(v) for v in values.values()) < 1:
            names = list(values)
            listed = names[0] if len(names) == 1 else ", ".join(names[:-1]) + " and " + names[-1]
            raise ValueError(f"{cls.KEY}: {listed} must be at least 1")

    def _refuse_capture(self):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__}.run: never inside a graph capture")

    # ---- what the driver calls --------------------------------------------------------------------------------------------
    def build_loaders(self, T: int, size: int, device, seed: int = 0) -> tuple:
        """The monitor's stand-in data as the tuple ``run`` takes behind the model; () for a monitor that reads the model alone."""
        return ()

    def run_epoch(self, model, loaders: tuple, ctx: dict) -> dict:
        """One due epoch on rank 0.  ctx: the driver's dict of this epoch -- "epoch", "num_epochs", "run_dir", "due" (the KEYs of the
        monitors due this epoch) -- in which a monitor may leave something for a later one."""
        return self.run(model, *loaders)

    def scalars(self, result: dict) -> dict:
        """The entries of the epoch's scalars.jsonl line."""
        raise NotImplementedError

    def log_line(self, result: dict, ctx: dict) -> str:
        raise NotImplementedError
