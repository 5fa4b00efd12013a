"""Episode traces (--trace_dir): the host side of the device flight recorder (rmbx_episode_trace,
include/rmbx.h; kernels.EpisodeTrace owns the device chunk).

A trace directory holds
  chunk_<seq>.npz   uncompressed; the rows the device recorded between two flushes, one array per
                    field (FIELDS), step-major and in slot order
  header.json       what the run was: policy, env, model, image size, cameras, seed, worlds, skip,
                    stride, camera settings, the dimensions
  episodes.npy      one record per episode of the run (_native.EPISODE_DTYPE), traced or not
and, under --num_gpus, one such directory rank<r>/ per rank.  A row holds the four arrays the
renderer reads (gxpos, gxmat, xpos, xquat), so any recorded step can be drawn again bit for bit
(bin/Replay.py), and the state beside them.

TraceWriter flushes the device chunk every 16 env-steps -- one host synchronisation, on the steps
the streaming loop polls anyway -- and hands the rows to one writer thread.  TraceReader indexes
the chunks of a directory (all ranks) by episode.  Neither needs a device for chunks given as
numpy arrays.
"""

import glob
import json
import os
import queue
import re
import threading

import numpy as np

FORMAT_VERSION = 1
POLL_STEPS = 16  # env-steps between two flushes (kernels.TRACE_POLL_STEPS: the chunk's capacity)
QUEUE_CHUNKS = 4  # flushed chunks that may wait for the writer thread

# field -> (dtype, per-row shape from the header's dimensions)
FIELDS = {
    "episode": (np.int32, lambda d: ()), "slot": (np.int32, lambda d: ()), "step": (np.int32, lambda d: ()),
    "phase": (np.int32, lambda d: ()), "rollout_time_idx": (np.int32, lambda d: ()), "flags": (np.uint8, lambda d: ()),
    "time": (np.float64, lambda d: ()), "reward": (np.float64, lambda d: ()),
    "ctrl": (np.float64, lambda d: (d["nu"],)), "qpos": (np.float64, lambda d: (d["nq"],)),
    "qvel": (np.float64, lambda d: (d["nv"],)), "gxpos": (np.float64, lambda d: (d["ngeom"], 3)),
    "gxmat": (np.float64, lambda d: (d["ngeom"], 9)), "xpos": (np.float64, lambda d: (d["nbody"], 3)),
    "xquat": (np.float64, lambda d: (d["nbody"], 4)),
}
FLAG_DONE, FLAG_SUCCESS, FLAG_BAD_STATE = 1, 2, 4  # include/rmbx.h RMBX_TRACE_*


def row_bytes(dims):
    """Bytes of one row for the dimensions {nq, nv, nu, ngeom, nbody}."""
    return int(sum(np.dtype(dt).itemsize * int(np.prod(shape(dims), dtype=np.int64)) for dt, shape in FIELDS.values()))


def parse_episodes(values):
    """--trace_episodes: None for `all`, else the sorted global episode indices."""
    if values is None:
        return None
    values = [values] if isinstance(values, (str, int)) else list(values)
    if len(values) == 1 and str(values[0]) == "all":
        return None
    try:
        out = sorted(set(int(v) for v in values))
    except ValueError:
        raise ValueError(f"--trace_episodes takes `all` or episode indices, not {values}") from None
    if not out or out[0] < 0:
        raise ValueError(f"--trace_episodes takes `all` or non-negative episode indices, not {values}")
    return out


def select_mask(episodes, episode_base, n_episodes):
    """u8 [n_episodes] mask of rmbx_episode_trace's `select` for the global indices `episodes` (None:
    no mask, every episode)."""
    if episodes is None:
        return None
    m = np.zeros(int(n_episodes), np.uint8)
    for i in episodes:
        if 0 <= i - episode_base < n_episodes:
            m[i - episode_base] = 1
    return m


class TraceWriter:
    """Writes one trace directory.  With `trace` (a kernels.EpisodeTrace) step() records an env-step
    on the device and flushes the chunk every POLL_STEPS calls; append() takes rows that are already
    host arrays.  finish() flushes the remainder, joins the writer thread and writes header.json and
    episodes.npy."""

    def __init__(self, directory, header, trace=None):
        self.directory = os.path.abspath(directory)
        os.makedirs(self.directory, exist_ok=True)
        if glob.glob(os.path.join(self.directory, "chunk_*.npz")):
            raise ValueError(f"{self.directory} already holds a trace: give --trace_dir a fresh directory")
        self.header = dict(header, format_version=FORMAT_VERSION)
        self.trace = trace
        self.calls = 0  # env-steps recorded
        self.seq = 0  # chunks handed to the thread
        self.rows_written = 0
        self.flush_seconds = []  # host time of every flush (scripts/prof_trace.py)
        self._error = None
        # bounded: a disk slower than the run holds the run back instead of filling pinned memory
        self._queue = queue.Queue(maxsize=QUEUE_CHUNKS)
        self._thread = threading.Thread(target=self._write_loop, name="trace-writer", daemon=True)
        self._thread.start()
        self._finished = False

    def _write_loop(self):
        while True:
            item = self._queue.get()
            if item is None:
                return
            seq, arrays = item
            if self._error is not None:
                continue  # keep draining so finish() never blocks
            try:
                path = os.path.join(self.directory, f"chunk_{seq:06d}.npz")
                with open(path + ".tmp", "wb") as f:
                    np.savez(f, **arrays)
                os.replace(path + ".tmp", path)
            except BaseException as e:  # reported by finish()
                self._error = e

    def append(self, arrays):
        """Queue the rows {field: array [rows, ...]} as the next chunk; None or no rows: nothing."""
        if self._finished:
            raise RuntimeError("the trace is finished")
        if arrays is None or len(arrays["episode"]) == 0:
            return
        missing = set(FIELDS) - set(arrays)
        if missing:
            raise ValueError(f"trace rows without the fields {sorted(missing)}")
        rows = len(arrays["episode"])
        for name in FIELDS:
            if len(arrays[name]) != rows or arrays[name].dtype != np.dtype(FIELDS[name][0]):
                raise ValueError(f"trace field {name}: {rows} rows of {np.dtype(FIELDS[name][0])} expected")
        self._queue.put((self.seq, {name: arrays[name] for name in FIELDS}))
        self.seq += 1
        self.rows_written += rows

    def step(self, stepped, reward):
        """Record one env-step on the device; every POLL_STEPS-th call flushes."""
        self.trace.record(stepped, reward)
        self.calls += 1
        if self.calls % POLL_STEPS == 0:
            self.flush()

    def flush(self):
        """Read the row counter, copy the used rows to pinned host memory, reset the counter and
        hand the rows to the writer thread (kernels.EpisodeTrace.flush)."""
        import time

        t0 = time.perf_counter()
        self.append(self.trace.flush())
        self.flush_seconds.append(time.perf_counter() - t0)

    def abort(self):
        """Stop the thread without writing the header (a run that was reset before it finished)."""
        if not self._finished:
            self._finished = True
            self._queue.put(None)
            self._thread.join()

    def finish(self, episodes):
        """episodes: the run's records (_native.EPISODE_DTYPE)."""
        if self._finished:
            raise RuntimeError("the trace is finished")
        try:
            if self.trace is not None:
                self.flush()
        finally:
            self.abort()
        if self._error is not None:
            raise RuntimeError(f"writing the trace to {self.directory} failed: {self._error!r}") from self._error
        self.header["chunks"], self.header["rows"] = self.seq, self.rows_written
        np.save(os.path.join(self.directory, "episodes.npy"), np.asarray(episodes))
        with open(os.path.join(self.directory, "header.json"), "w") as f:
            json.dump(self.header, f, indent=1, sort_keys=True)


def _trace_dirs(directory):
    ranks = []
    for p in glob.glob(os.path.join(directory, "rank*")):
        m = re.fullmatch(r"rank(\d+)", os.path.basename(p))
        if m and os.path.isdir(p):
            ranks.append((int(m.group(1)), p))
    if ranks:
        return [p for _, p in sorted(ranks)]
    return [directory]


class TraceReader:
    """Index of a trace directory (of all its rank<r>/ directories, if it has them) by episode."""

    def __init__(self, directory):
        self.directory = os.path.abspath(directory)
        self.dirs = _trace_dirs(self.directory)
        self.headers = []
        records = []
        self._index = {}  # episode -> [(chunk path, row indices)]
        for d in self.dirs:
            hp = os.path.join(d, "header.json")
            if not os.path.exists(hp):
                raise ValueError(f"{d} is not a finished trace: no header.json")
            with open(hp) as f:
                h = json.load(f)
            if h.get("format_version") != FORMAT_VERSION:
                raise ValueError(f"{hp}: trace format {h.get('format_version')}, this reader reads {FORMAT_VERSION}")
            self.headers.append(h)
            records.append(np.load(os.path.join(d, "episodes.npy")))
            for path in sorted(glob.glob(os.path.join(d, "chunk_*.npz"))):
                with np.load(path) as z:
                    ep = z["episode"]
                for e in np.unique(ep):
                    self._index.setdefault(int(e), []).append((path, np.nonzero(ep == e)[0]))
        self.header = self.headers[0]
        rec = np.concatenate(records)
        rec = rec[rec["episode"] >= 0]
        self.episodes = rec[np.argsort(rec["episode"], kind="stable")]

    @property
    def traced_episodes(self):
        """The episodes that have rows, sorted."""
        return sorted(self._index)

    def record(self, i):
        """The record of episode i (a row of `episodes`)."""
        hit = np.nonzero(self.episodes["episode"] == int(i))[0]
        if len(hit) == 0:
            raise ValueError(f"episode {i} is not part of the run in {self.directory} "
                             f"({len(self.episodes)} episodes recorded)")
        return self.episodes[hit[0]]

    def episode(self, i):
        """The rows of episode i in step order: {field: array [rows, ...]}."""
        parts = self._index.get(int(i))
        if parts is None:
            some = self.traced_episodes
            shown = ", ".join(str(e) for e in some[:20]) + (", ..." if len(some) > 20 else "")
            raise ValueError(f"episode {i} has no rows in {self.directory}; traced episodes: {shown or 'none'}")
        out = {name: [] for name in FIELDS}
        for path, rows in parts:
            with np.load(path) as z:
                for name in FIELDS:
                    out[name].append(z[name][rows])
        out = {name: np.concatenate(v) for name, v in out.items()}
        order = np.argsort(out["step"], kind="stable")
        return {name: np.ascontiguousarray(v[order]) for name, v in out.items()}
