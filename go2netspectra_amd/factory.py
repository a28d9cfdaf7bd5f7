"""Aggregator registry and the batch Manager.

Reference: internal/factory/task_factory.go:12-52 (TaskGroup, RegisterAggregator
panics on duplicates, Create builds groups from aggregator.types) and
internal/engine/manager/manager.go (worker pool, snapshotter, resetter).

The Manager keeps the reference's lifecycle (start -> packets -> snapshot /
reset -> stop) but replaces the goroutine worker pool fed one *PacketInfo at a
time (manager.go:218-244) with batch submission: every task receives each
packet batch in arrival order on its GPU stream.  Writers (ClickHouse / text),
alerting and the timers are out of scope for this build.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List

from .config import Config
from .task import SketchTask


@dataclass
class TaskGroup:
    Tasks: List[SketchTask] = field(default_factory=list)
    Writers: List[object] = field(default_factory=list)


TaskFactory = Callable[[Config], TaskGroup]
_registry: Dict[str, TaskFactory] = {}


def register_aggregator(name: str, factory: TaskFactory) -> None:
    if name in _registry:  # task_factory.go:25-27 panics
        raise RuntimeError(f"aggregator type '{name}' already registered")
    _registry[name] = factory


def create(cfg: Config, **task_kw) -> List[TaskGroup]:
    groups = []
    for agg in cfg.Aggregator.Types:
        f = _registry.get(agg)
        if f is None:
            raise KeyError(f"unknown aggregator type: '{agg}'")
        groups.append(f(cfg, **task_kw))
    return groups


def _sketch_factory(cfg: Config, **task_kw) -> TaskGroup:  # sketch/task.go:21-65
    return TaskGroup(Tasks=[SketchTask(t, **task_kw) for t in cfg.Aggregator.Sketch.Tasks], Writers=[])


def _exact_factory(cfg: Config, device: int = 0, max_flows: int = 0, batch_packets: int = 0,
                   **_sketch_only) -> TaskGroup:  # exact/task.go:20-64
    from .exact import ExactTask
    return TaskGroup(Tasks=[ExactTask(t.Name, t.KeyFields, t.NumShards, device=device, max_flows=max_flows,
                                      batch_packets=batch_packets) for t in cfg.Aggregator.Exact.Tasks], Writers=[])


register_aggregator("sketch", _sketch_factory)
register_aggregator("exact", _exact_factory)
RegisterAggregator = register_aggregator
Create = create


def key_fields(task) -> List[str]:
    """The fields a task keys its flows on: FlowFields (sketch, task.go:265-300) or
    KeyFields (exact, exact/task.go:330-366)."""
    if hasattr(task, "flow_fields"):
        return list(task.flow_fields)
    return list(task.agg.key_fields)


class Manager:
    """Batch-submission replacement of manager.Manager."""

    def __init__(self, cfg: Config, **task_kw):
        self.groups = create(cfg, **task_kw)
        self.device = int(task_kw.get("device", 0))
        self.started = False

    def tasks(self) -> List[SketchTask]:
        return [t for g in self.groups for t in g.Tasks]

    def start(self) -> None:
        self.started = True

    def owner_fields(self) -> List[str]:
        """The owner key for sharding this Manager's tasks over GPUs (dist.owner_fields):
        every task sees every packet (manager.go:232-244), so one owner must hold
        each flow of every task.  Raises ValueError when the tasks share no key field."""
        from .dist import owner_fields
        return owner_fields([key_fields(t) for t in self.tasks()])

    def process(self, batch) -> None:
        """processPacket (manager.go:232-244) for a whole batch: fan out to every task.
        A host CompactBatch is uploaded once and every task reads the device copy
        (each task would otherwise stage its own)."""
        from .packets import CompactBatch
        if isinstance(batch, CompactBatch) and not batch.is_device() and len(self.tasks()) > 1 and len(batch):
            import torch
            batch = batch.to(torch.device("cuda", self.device))
        for t in self.tasks():
            t.process_packets(batch)

    def snapshot(self) -> Dict[str, object]:
        """takeSnapshotForWriter without writers: name -> HeavyRecord (sketch) / SnapshotData (exact)."""
        return {t.name(): t.snapshot() for t in self.tasks()}

    def views(self) -> List[object]:
        """One snapshot view per task, in tasks() order (CountMinView, SuperSpreadView,
        ExactView): the read side of the snapshotter / alerter thread."""
        return [t.view() for t in self.tasks()]

    def refresh_views(self, views, state: bool = False, detach: bool = False) -> None:
        """Ingest side: refresh every view at this point of the stream (asynchronous).
        state=True: the SuperSpread views also capture what a checkpoint needs.
        detach=True: the Count-Min views take detached snapshots, which stay readable
        across reset_all() and can be checkpointed (save_from)."""
        from .sketch import CountMinView, SuperSpreadView
        for v in views:
            if isinstance(v, SuperSpreadView):
                v.refresh(state=state)
            elif isinstance(v, CountMinView):
                v.refresh(detach=detach)
            else:
                v.refresh()

    def snapshot_from_views(self, views) -> Dict[str, object]:
        """snapshot() as of the views' last refresh; may run on another thread while
        process() keeps feeding the tasks."""
        return {t.name(): t.snapshot_from(v) for t, v in zip(self.tasks(), views)}

    def keep_history(self, retain=None, **kw) -> Dict[str, object]:
        """ExactTask.keep_history for every exact task: name -> ExactHistory.  ``retain=N``: each
        record folds the task's history down to at most N snapshots (None: keep everything)."""
        return {t.name(): t.keep_history(retain=retain, **kw) for t in self.tasks() if hasattr(t, "keep_history")}

    def record(self, timestamp_ns: int, full: bool = False) -> Dict[str, object]:
        """One snapshot interval: every exact task's changed flows into its history under ONE
        timestamp, as the reference's snapshotter writes them (manager.go:140).  name -> (rows
        appended, keys new to the history)."""
        tasks = [t for t in self.tasks() if hasattr(t, "record")]
        for t in tasks:
            if getattr(t, "history", None) is None:
                raise ValueError(f"record: task {t.name()} has no history (keep_history first)")
        return {t.name(): t.record(timestamp_ns, full=full) for t in tasks}

    def keep_heavy_history(self, retain=None, drop: bool = False, **kw) -> Dict[str, object]:
        """SketchTask.keep_heavy_history for every sketch task: name -> HeavyHistory.  ``retain=N``:
        each record_heavy trims the task's history to the newest N snapshots, folding the older
        ones into a base (``drop=True``: dropping them); None keeps everything."""
        return {t.name(): t.keep_heavy_history(retain=retain, drop=drop, **kw) for t in self.tasks()
                if hasattr(t, "keep_heavy_history")}

    def record_heavy(self, timestamp_ns: int) -> Dict[str, object]:
        """One interval of the sketch writers: every sketch task's lists into its heavy history
        under ONE timestamp.  The reference runs one snapshotter per writer, so this timestamp
        is separate from the exact tasks' ``record``.  name -> (rows appended, pairs new)."""
        tasks = [t for t in self.tasks() if hasattr(t, "record_heavy")]
        for t in tasks:
            if getattr(t, "heavy_history", None) is None:
                raise ValueError(f"record_heavy: task {t.name()} has no heavy history (keep_heavy_history first)")
        return {t.name(): t.record_heavy(timestamp_ns) for t in tasks}

    def reset_all(self) -> None:  # resetAllTasks, manager.go:179-193
        for t in self.tasks():
            t.reset()

    def checkpoint(self, dir) -> List[str]:
        """Every task's state into ``dir``, one file per task name (task.save), then
        ``<name>.history.npz`` for each task that has a history attached (its whole log), then
        ``<name>.heavy.npz`` for each sketch task that has a heavy history attached; returns the
        paths, the history files after the task files."""
        import os
        os.makedirs(dir, exist_ok=True)
        paths = []
        for t in self.tasks():
            paths.append(os.path.join(dir, t.name() + ".npz"))
            t.save(paths[-1])
        for t in self.tasks():
            if getattr(t, "history", None) is not None:
                paths.append(os.path.join(dir, t.name() + ".history.npz"))
                t.save_history(paths[-1])
        for t in self.tasks():
            if getattr(t, "heavy_history", None) is not None:
                paths.append(os.path.join(dir, t.name() + ".heavy.npz"))
                t.save_heavy_history(paths[-1])
        return paths

    def restore(self, dir) -> None:
        """Every task's state from the files ``checkpoint`` wrote into ``dir`` (task.restore):
        the tasks must be configured as the saved ones were.  A task with a history attached
        also takes back ``<name>.history.npz`` when that file exists, so ``end_time`` answers
        survive the restart.  The next delta ``record`` then stores every restored flow again
        -- the merge that restored the table touched them all -- which is correct, only larger."""
        import os
        for t in self.tasks():
            t.restore(os.path.join(dir, t.name() + ".npz"))
            hp = os.path.join(dir, t.name() + ".history.npz")
            if getattr(t, "history", None) is not None and os.path.exists(hp):
                t.restore_history(hp)
            vp = os.path.join(dir, t.name() + ".heavy.npz")
            if getattr(t, "heavy_history", None) is not None and os.path.exists(vp):
                t.restore_heavy_history(vp)

    def stop(self) -> Dict[str, object]:
        """Drain (flush every stream) and take the final snapshot (manager.go:196-216)."""
        for t in self.tasks():
            t.flush()
        self.started = False
        return self.snapshot()
