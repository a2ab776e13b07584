"""Net health for a training loop: is the weight table still one the value net can play with, is its hidden layer saturated, and do
the candidates of a turn still get different values?  (include/bgamd.h: bgamd_net_health, bgamd_env_choice_spread; the kernels are in
csrc/bg_health.h.  Everything is measured on the device; the host reads one 576-byte struct.)

    h = net_health(learner.theta, health_rows(traj, lengths, steps))       # or learner.health(rows); round_rows(traj, lengths, n):
                                                                           # n rows spread over all the round's turns
    s = env.choice_spread()                                                # after a greedy step
    check(h, s, max_saturated_share=..., max_all_tied_share=...)           # raises NetHealthError naming what failed

THRESHOLD = 15: sigmoid'(15) ~ 3e-7 -- a hidden unit that far out passes no gradient and gives every row the same output."""
from __future__ import annotations

import ctypes as C

import torch

from . import _capi

THRESHOLD = 15.0
TENSORS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
N_HID = 128


class NetHealthError(RuntimeError):
    """check() found the table unusable or past a limit; .failed lists (condition, number, limit) for every condition that failed."""

    def __init__(self, failed):
        self.failed = list(failed)
        super().__init__("net health: " + "; ".join(m for m, _, _ in self.failed))


def net_health(theta, rows=None, threshold: float = THRESHOLD) -> dict:
    """theta: float32 [25601] (W1[128,198] | b1 | W2 | b2; moved to the device when it is not there), rows: int32 [..., 8] 32-byte rows
    (pack_rows, a trajectory log, health_rows) or None.  -> dict: nonfinite, rows, saturated, dead_units, saturated_share (of rows x 128
    pairs; 0.0 without rows), max_abs {tensor: largest finite |w|}, max_abs_preact, v_min, v_max, fits_f16_split (bool),
    unit_saturated (int32 [128] tensor, on the device).  The activation fields mean something only when nonfinite == 0.
    Synchronises (the struct is read back)."""
    lib = _capi.load()
    if not torch.cuda.is_available():
        raise _capi.BgamdError("no GPU visible: backgammon_env has no CPU fallback")
    th = torch.as_tensor(theta, dtype=torch.float32).flatten()
    if th.numel() != 25601:
        raise ValueError("expected 25601 weights (198->128->1)")
    if not th.is_cuda:
        th = th.cuda()
    th = th.contiguous()
    r, n = None, 0
    if rows is not None:
        r = torch.as_tensor(rows, dtype=torch.int32).to(th.device).reshape(-1, 8).contiguous()
        n = int(r.shape[0])
    out = torch.empty(C.sizeof(_capi.NetHealth), dtype=torch.uint8, device=th.device)
    with torch.cuda.device(th.device):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _capi.check(lib.bgamd_net_health(C.c_void_p(th.data_ptr()), C.c_void_p(r.data_ptr()) if n else None, n, float(threshold),
                                         C.c_void_p(out.data_ptr()), stream), "net_health")
        raw = out.cpu().numpy().tobytes()                      # (waits for the stream)
    h = _capi.NetHealth.from_buffer_copy(raw)
    off = _capi.NetHealth.unit_saturated.offset
    units = out[off:off + 4 * N_HID].view(torch.int32)
    return {"nonfinite": int(h.nonfinite), "rows": int(h.rows), "saturated": int(h.saturated), "dead_units": int(h.dead_units),
            "saturated_share": (h.saturated / (h.rows * float(N_HID))) if h.rows else 0.0,
            "max_abs": {k: float(v) for k, v in zip(TENSORS, h.max_abs)}, "max_abs_preact": float(h.max_abs_preact),
            "v_min": float(h.v_min), "v_max": float(h.v_max), "fits_f16_split": bool(h.fits_f16_split),
            "unit_saturated": units, "threshold": float(threshold)}


def health_rows(traj, lengths, steps):
    """From a [T, n, 8] trajectory log (play_round) the rows of the given steps that lie inside their games: step t of lane g counts iff
    t < lengths[g].  The log is zero beyond a game's end (and for lanes that are not replayed, lengths 0): such padding rows are never
    selected -- an all-zero row is an empty board the net would be measured on otherwise.  -> int32 [m, 8]"""
    T = int(traj.shape[0])
    st = torch.as_tensor(steps, dtype=torch.int64, device=traj.device).flatten()
    st = st[(st >= 0) & (st < T)]
    inside = st[:, None] < torch.as_tensor(lengths, device=traj.device).to(torch.int64)[None, :]
    return traj[st][inside].reshape(-1, 8).contiguous()


def thin(rows, n_rows: int):
    """At most n_rows of rows [m, 8], evenly spaced over all m (not the first n_rows: a log is step-major, its head is one step)."""
    m, k = int(rows.shape[0]), int(n_rows)
    if m <= k:
        return rows
    return rows[(torch.arange(k, device=rows.device, dtype=torch.int64) * m) // k].contiguous()


def round_rows(traj, lengths, n_rows: int):
    """n_rows rows of a [T, n, 8] log spread evenly over ALL the round's turns: the turns inside their games (t < lengths[g], as
    health_rows), counted step by step, every (turns / n_rows)-th of them.  A step gets rows in proportion to the lanes still playing at
    it, so with n_rows = n a round is covered from its first turn to where fewer than one mean game length of lanes are left -- not its
    first step alone.  Padding is never selected; n_rows >= the round's turns returns every turn once.  -> int32 [m, 8]"""
    T, n = int(traj.shape[0]), int(traj.shape[1])
    dev = traj.device
    ln = torch.as_tensor(lengths, device=dev).to(torch.int64).flatten().clamp(0, T)
    if T == 0 or n == 0 or int(n_rows) <= 0:
        return traj.new_zeros((0, 8))
    order = torch.argsort(ln, descending=True, stable=True)            # the lanes inside their game at step t are order[:live[t]]
    live = n - torch.searchsorted(ln.sort().values, torch.arange(T, device=dev), right=True)
    cum = live.cumsum(0)
    total = int(cum[-1].item())
    m = min(int(n_rows), total)
    if m == 0:
        return traj.new_zeros((0, 8))
    j = (torch.arange(m, device=dev, dtype=torch.int64) * total) // m   # the j-th turn of the round in (step, remaining lanes) order
    t = torch.searchsorted(cum, j, right=True)
    return traj[t, order[j - (cum[t] - live[t])]].reshape(-1, 8).contiguous()


def all_tied_share(spread) -> float:
    """Of the lanes that had a choice (>= 2 rows), the share whose rows all had the same value: the tie rule alone moved there."""
    return spread["all_tied_lanes"] / spread["choice_lanes"] if spread["choice_lanes"] else 0.0


def check(health, spread=None, max_saturated_share=None, max_all_tied_share=None, min_choice_lanes: int = 1):
    """Raises NetHealthError naming every condition that failed, with its number.  Always: nonfinite > 0 and fits_f16_split == 0
    (load_weights would refuse that table: BGAMD_E_WEIGHTS).  Optional limits: saturated_share of the measured rows, and the all-tied
    share of `spread` (VecGame.choice_spread()) when at least min_choice_lanes lanes had a choice (a share of a handful of lanes says
    nothing about the net)."""
    failed = []
    if health["nonfinite"] > 0:
        failed.append(("%d of 25601 weights are not finite" % health["nonfinite"], health["nonfinite"], 0))
    if not health["fits_f16_split"]:
        failed.append(("the table does not fit the value net's f16 hi + lo planes (largest finite |fc1.weight| %.6g, bound 65504): "
                       "load_weights would refuse it" % health["max_abs"]["fc1.weight"], health["max_abs"]["fc1.weight"], 65504.0))
    if max_saturated_share is not None and health["saturated_share"] > max_saturated_share:
        failed.append(("saturated share %.4f of %d rows x 128 units (|a| > %g) is above the limit %.4f; %d dead units"
                       % (health["saturated_share"], health["rows"], health.get("threshold", THRESHOLD), max_saturated_share,
                          health["dead_units"]), health["saturated_share"], max_saturated_share))
    if (max_all_tied_share is not None and spread is not None and spread["choice_lanes"] >= max(1, int(min_choice_lanes))
            and all_tied_share(spread) > max_all_tied_share):
        failed.append(("all candidates tie in %d of %d lanes with a choice (share %.4f) -- above the limit %.4f"
                       % (spread["all_tied_lanes"], spread["choice_lanes"], all_tied_share(spread), max_all_tied_share),
                       all_tied_share(spread), max_all_tied_share))
    if failed:
        raise NetHealthError(failed)


def line(health, spread=None) -> str:
    """One line for a training loop's log."""
    m = health["max_abs"]
    s = ("health: max|theta| fc1.w %.4g fc1.b %.4g fc2.w %.4g fc2.b %.4g, nonfinite %d, saturated share %.4f on %d rows "
         "(max|a| %.4g, dead units %d, values %.4f .. %.4f)"
         % (m["fc1.weight"], m["fc1.bias"], m["fc2.weight"], m["fc2.bias"], health["nonfinite"], health["saturated_share"], health["rows"],
            health["max_abs_preact"], health["dead_units"], health["v_min"], health["v_max"]))
    if spread is not None:
        s += ", all-tied share %.4f of %d lanes with a choice" % (all_tied_share(spread), spread["choice_lanes"])
    return s
