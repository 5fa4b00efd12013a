"""Host side of --episode_metrics: the table of rmbx_episode_metrics (include/rmbx.h, one row per
episode, accumulated on the device) as result lists and as a printed summary.

No device work here: the rows arrive as a structured numpy array (_native.METRICS_DTYPE)."""

import math

import numpy as np

from .. import _native as N

# the row fields reported per episode (all but `episode`), in the row's order
INT_FIELDS = ("steps", "first_success_step", "flags")
F64_FIELDS = ("peak_force", "peak_torque", "peak_joint_speed", "peak_tracking_error", "ee_path", "joint_path",
              "cmd_roughness")
# result["metrics"]: the row fields, and first_success_step in seconds beside it
RESULT_KEYS = ("steps", "first_success_step", "first_success_time", "flags") + F64_FIELDS
# the columns of the multi-GPU gather: the whole row, then the episode's world index
TABLE_COLUMNS = ("episode",) + INT_FIELDS + F64_FIELDS + ("world_idx",)

Z95 = 1.959963984540054  # the 97.5 % point of the standard normal


def wilson_interval(successes, n, z=Z95):
    """Wilson score interval (lo, hi) of a binomial proportion successes / n; (0, 1) for n == 0."""
    n, k = int(n), int(successes)
    if n <= 0:
        return 0.0, 1.0
    p, z2 = k / n, z * z
    denom = 1.0 + z2 / n
    centre = (p + z2 / (2 * n)) / denom
    half = z * math.sqrt(p * (1.0 - p) / n + z2 / (4.0 * n * n)) / denom
    return max(0.0, centre - half), min(1.0, centre + half)


def table_to_columns(table, world_idx):
    """[n, len(TABLE_COLUMNS)] f64 of a metrics table and the episodes' world indices: the form the
    rows are all-gathered in (every value is exact in f64)."""
    cols = [np.asarray(table[f], np.float64) for f in TABLE_COLUMNS[:-1]]
    cols.append(np.asarray(world_idx, np.float64).reshape(len(table)))
    return np.stack(cols, axis=1) if len(table) else np.zeros((0, len(TABLE_COLUMNS)))


def columns_to_table(cols):
    """(table, world_idx) back from table_to_columns' form."""
    cols = np.asarray(cols, np.float64).reshape(-1, len(TABLE_COLUMNS))
    table = np.zeros(len(cols), dtype=N.METRICS_DTYPE)
    for i, f in enumerate(TABLE_COLUMNS[:-1]):
        table[f] = cols[:, i]
    return table, cols[:, -1].astype(np.int64)


def metrics_result(table, step_seconds):
    """result["metrics"]: {field: per-episode list}, parallel to result["success"].
    first_success_time is first_success_step in seconds (0.0 = never)."""
    out = {}
    for f in INT_FIELDS:
        out[f] = [int(x) for x in table[f]]
    out["first_success_time"] = [float(x) * float(step_seconds) for x in table["first_success_step"]]
    for f in F64_FIELDS:
        out[f] = [float(x) for x in table[f]]
    return {k: out[k] for k in RESULT_KEYS}


def _stats(x):
    """(mean, median, 95th percentile) of a 1-D array, None when it is empty."""
    x = np.asarray(x, np.float64)
    if x.size == 0:
        return None
    return float(np.mean(x)), float(np.median(x)), float(np.percentile(x, 95))


def summarize(table, success, world_idx, step_seconds):
    """The figures of the printed summary as a dict: counted / successful episode counts, success
    rate with its Wilson 95 % interval, success per world index, and (mean, median, p95) of every
    metric over the counted episodes ("all") and over the successful ones ("success").  An episode
    is counted when its row is not empty (steps > 0); first_success_time is over the episodes that
    have one."""
    success = np.asarray(success, bool).reshape(len(table))
    world_idx = np.asarray(world_idx, np.int64).reshape(len(table))
    counted = table["steps"] > 0
    n, k = len(table), int(success.sum())
    per_world = {int(w): (int(success[world_idx == w].sum()), int((world_idx == w).sum()))
                 for w in sorted(set(world_idx.tolist()))}
    stats = {}
    for f in ("steps",) + F64_FIELDS:
        stats[f] = {"all": _stats(table[f][counted]), "success": _stats(table[f][counted & success])}
    t = table["first_success_step"].astype(np.float64) * float(step_seconds)
    has = counted & (table["first_success_step"] > 0)
    stats["first_success_time"] = {"all": _stats(t[has]), "success": _stats(t[has & success])}
    return {"episodes": n, "counted": int(counted.sum()), "successes": k, "success_rate": k / n if n else 0.0,
            "wilson95": wilson_interval(k, n), "per_world": per_world,
            "flagged": int((table["flags"] & N.METRICS_BAD_STATE != 0).sum()), "stats": stats}


_UNITS = {"steps": "", "first_success_time": " [s]", "peak_force": " [N]", "peak_torque": " [N m]",
          "peak_joint_speed": " [rad/s]", "peak_tracking_error": " [rad]", "ee_path": " [m]", "joint_path": " [rad]",
          "cmd_roughness": " [rad^2]"}


def summary_lines(summary):
    """The summary as the lines print_statistics adds."""
    s = summary
    lo, hi = s["wilson95"]
    lines = [f"  - Episode metrics | {s['counted']} of {s['episodes']} episodes counted, {s['successes']} successful, "
             f"{s['flagged']} stopped by a bad-state reset",
             f"  - Success rate | {s['success_rate']:.4f} ({s['successes']}/{s['episodes']}), Wilson 95% interval "
             f"[{lo:.4f}, {hi:.4f}]",
             "  - Success per world index | " + ", ".join(f"{w}: {a}/{b}" for w, (a, b) in s["per_world"].items())]

    def fmt(v):
        return "none" if v is None else f"mean: {v[0]:.4e}, median: {v[1]:.4e}, p95: {v[2]:.4e}"

    for f in ("steps", "first_success_time") + F64_FIELDS:
        st = s["stats"][f]
        lines.append(f"  - {f}{_UNITS[f]} | all | {fmt(st['all'])} | successful | {fmt(st['success'])}")
    return lines
