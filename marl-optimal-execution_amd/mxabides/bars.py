"""Time bars from the book-update log, replayed on the device (include/mxa_bars.h).

One kernel launch turns every env's 16-byte record stream (include/mxa.h mxa_book_rec, the input of
mxabides.booklog) into bars [n_envs][n_bars][12] int64 on a time grid: the inside quotes at each
bar's close, the trade open / high / low / close, volume, notional and counts: the series the
reference's cli/event_midpoint.py and realism/ read from the exchange's BEST_BID / BEST_ASK /
LAST_TRADE rows.  VecMarket.write_bars / VecMarket.bars run it on a handle's own log; from_records
runs it on records a caller holds in device tensors."""
import ctypes

import numpy as np

from . import _lib

WORDS = 12         # include/mxa_bars.h MXA_BAR_WORDS
STATUS_WORDS = 4   # MXA_BAR_STATUS_WORDS
MAX_LEVELS = 1024  # MXA_BAR_MAX_LEVELS
COLUMNS = ("bid", "bid_size", "ask", "ask_size", "open", "high", "low", "close", "volume", "notional",
           "executed_orders", "records")
STATUS_COLUMNS = ("code", "records_consumed", "peak_bid_levels", "peak_ask_levels")
# status codes
OK, LOG_OVERFLOW, LEVELS_EXCEEDED, STREAM_INCONSISTENT = 0, 1, 2, 3


def from_records(rec, counts, level_cap, t0_ns, dt_ns, n_bars, stream=None):
    """(bars [n_envs, n_bars, 12] int64, status [n_envs, 4] int32) torch device tensors from records on
    the device: rec [n_envs, rec_stride, 4] int32 (or [n_envs, rec_stride, 2] int64: mxa_book_rec rows
    viewed as words), counts [n_envs] int32.  Asynchronous on `stream` (a torch.cuda.Stream; None: the
    current one); include/mxa_bars.h mxa_bars_from_records."""
    import torch
    L = _lib.load()
    if rec.dim() != 3 or rec.shape[2] * rec.element_size() != 16 or not rec.is_contiguous() or not rec.is_cuda:
        raise ValueError("rec: a contiguous device tensor [n_envs, rec_stride] of 16-byte records")
    n_envs, stride = int(rec.shape[0]), int(rec.shape[1])
    if counts.dtype != torch.int32 or counts.numel() != n_envs or not counts.is_contiguous() or counts.device != rec.device:
        raise ValueError("counts: a contiguous int32 tensor [n_envs] on rec's device")
    st = stream if stream is not None else torch.cuda.current_stream(rec.device)
    with torch.cuda.device(rec.device), torch.cuda.stream(st):
        bars = torch.empty((n_envs, max(int(n_bars), 0), WORDS), dtype=torch.int64, device=rec.device)
        status = torch.empty((n_envs, STATUS_WORDS), dtype=torch.int32, device=rec.device)
        rc = L.mxa_bars_from_records(ctypes.c_void_p(st.cuda_stream), n_envs, ctypes.c_void_p(rec.data_ptr()), stride,
                                     ctypes.c_void_p(counts.data_ptr()), int(level_cap), int(t0_ns), int(dt_ns), int(n_bars),
                                     ctypes.c_void_p(bars.data_ptr()) if bars.numel() else None,
                                     ctypes.c_void_p(status.data_ptr()))
    if rc < 0:
        raise _lib.MxaError("mxa_bars_from_records failed (%d): %s" % (rc, L.mxa_last_error(None).decode()))
    return bars, status


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def mid(bars):
    """(bid + ask) / 2 per bar as float64, NaN where a side is empty"""
    b = _np(bars)
    out = (b[..., 0] + b[..., 2]) / 2.0
    out[(b[..., 1] == 0) | (b[..., 3] == 0)] = np.nan
    return out


def vwap(bars):
    """notional / volume per bar as float64, NaN without a trade"""
    b = _np(bars)
    v = b[..., 8].astype(np.float64)
    out = np.full(v.shape, np.nan)
    np.divide(b[..., 9].astype(np.float64), v, out=out, where=v != 0)
    return out
