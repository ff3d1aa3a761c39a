"""Snapshots of whole markets: the blob cda_snapshot_pack builds on the device (include/cda.h, csrc/cda_snapshot.inc), its header, and snapshot files.

A `Snapshot` is the device (or host) uint8 blob plus its header as a dict.  `CDAVecEnv.snapshot()` makes one, `CDAVecEnv.restore()` puts markets of
one back into an env - the same one, or another with the same numeric config (a fork).  `save_snapshot` / `load_snapshot` write and read a single
torch.save dict with a format tag and version, like the policy files (mlp.policy_record); a file validates without a GPU."""
import ctypes as C

import torch

from . import _capi as K

SNAPSHOT_FORMAT = "cda-env-snapshot"
SNAPSHOT_FILE_VERSION = 1
HEADER_BYTES = C.sizeof(K.SnapshotHeader)          # 256

# fields of the header that must agree with the env a blob is restored into (book_spill may differ: the window is rebased)
_CFG_FIELDS = [n for n, _ in K.Config._fields_ if n not in ("book_spill", "book_capacity")]


def table_bytes(n_markets):
    """bytes of header + offset table of a blob of n markets (cda_snapshot_table_bytes, restated for the host)"""
    return 256 + ((8 * (int(n_markets) + 1) + 255) & ~255)


def parse_header(raw):
    """the first 256 bytes of a blob (bytes, numpy or CPU uint8 tensor) -> dict; ValueError when it is not a snapshot header this build reads"""
    if isinstance(raw, torch.Tensor):
        raw = raw.detach().cpu().contiguous().numpy().tobytes()
    raw = bytes(raw)
    if len(raw) < HEADER_BYTES:
        raise ValueError(f"a snapshot blob holds at least its {HEADER_BYTES}-byte header, got {len(raw)} bytes (truncated)")
    h = K.SnapshotHeader.from_buffer_copy(raw[:HEADER_BYTES])
    if h.magic != K.SNAP_MAGIC:
        raise ValueError(f"not a snapshot blob (magic {h.magic:#010x}, want {K.SNAP_MAGIC:#010x})")
    if h.version != K.SNAP_VERSION:
        raise ValueError(f"snapshot blob version {h.version} is not supported (this build reads version {K.SNAP_VERSION})")
    if h.n_markets < 1 or h.header_bytes != table_bytes(h.n_markets) or h.total_bytes < h.header_bytes:
        raise ValueError(f"corrupt snapshot header (n_markets {h.n_markets}, header_bytes {h.header_bytes}, total_bytes {h.total_bytes})")
    out = {n: getattr(h, n) for n, _ in K.SnapshotHeader._fields_ if n not in ("cfg", "reserved")}
    out["cfg"] = {n: getattr(h.cfg, n) for n, _ in K.Config._fields_}
    return out


class Snapshot:
    """A snapshot blob (uint8 tensor, device or CPU) and its parsed header.  len(snap) = markets it holds."""

    def __init__(self, blob, header, market_params=None):
        self.blob = blob
        self.header = header
        self.market_params = market_params      # the rows of its markets (numpy, market_params.ROW_DTYPE), or None: the markets ran the env's config

    def __len__(self):
        return int(self.header["n_markets"])

    @property
    def nbytes(self):
        return int(self.header["total_bytes"])

    def to(self, device):
        return Snapshot(self.blob.to(device), self.header, self.market_params)


def mismatch(header, env):
    """the first field in which a blob's header and an env disagree (a ValueError message naming it), or None"""
    want = {"book_capacity": env.book_capacity, "n_hist": env.n_hist, "num_agents": env.num_agents, "record_stride": env.state_bytes_per_market(),
            "episode_metrics_on": int(bool(getattr(env, "episode_metrics_on", False)))}
    for k, v in want.items():
        if int(header[k]) != int(v):
            return f"snapshot {k} = {header[k]}, the env has {v}"
    for k in _CFG_FIELDS:
        a, b = header["cfg"][k], getattr(env.cfg_struct, k)
        if a != b:
            return f"snapshot config {k} = {a}, the env has {b}"
    if header["episode_metrics_on"] and header["nav_tolerance"] != getattr(env, "episode_metrics_tolerance", header["nav_tolerance"]):
        return f"snapshot episode-metrics nav_tolerance = {header['nav_tolerance']}, the env has {env.episode_metrics_tolerance}"
    return None


def snapshot_record(snap):
    """the dict a snapshot file holds: {"format", "version", "header", "blob" (uint8, CPU)} and, for markets with rows of their own, "market_params"
    (uint8 [n, row bytes]: their cda_market_params rows)"""
    rec = {"format": SNAPSHOT_FORMAT, "version": SNAPSHOT_FILE_VERSION, "header": dict(snap.header), "blob": snap.blob.detach().to("cpu").contiguous().clone()}
    if snap.market_params is not None:
        import numpy as np
        rows = np.ascontiguousarray(snap.market_params)
        rec["market_params"] = torch.from_numpy(rows.view(np.uint8).reshape(len(rows), rows.dtype.itemsize).copy())
    return rec


def check_snapshot_record(rec):
    """validate a snapshot file's dict (format tag, version, blob against its header); returns the Snapshot (blob on the CPU)"""
    if not isinstance(rec, dict) or rec.get("format") != SNAPSHOT_FORMAT:
        raise ValueError(f"not a snapshot file (format tag {rec.get('format') if isinstance(rec, dict) else type(rec).__name__!r}, want {SNAPSHOT_FORMAT!r})")
    if rec.get("version") != SNAPSHOT_FILE_VERSION:
        raise ValueError(f"snapshot file version {rec.get('version')!r} is not supported (this build reads version {SNAPSHOT_FILE_VERSION})")
    blob = rec.get("blob")
    if not isinstance(blob, torch.Tensor) or blob.dtype != torch.uint8 or blob.dim() != 1:
        raise ValueError("a snapshot file's blob must be a 1-d uint8 tensor")
    header = parse_header(blob[:HEADER_BYTES])
    if blob.numel() != header["total_bytes"]:
        raise ValueError(f"snapshot blob holds {blob.numel()} bytes, its header says {header['total_bytes']} (truncated or padded)")
    if rec.get("header") != header:
        raise ValueError("a snapshot file's header record does not match the blob's own header")
    rows = rec.get("market_params")
    if rows is not None:
        from .market_params import ROW_DTYPE
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.uint8 or tuple(rows.shape) != (header["n_markets"], ROW_DTYPE.itemsize):
            raise ValueError(f"a snapshot file's market_params must be uint8 [{header['n_markets']}, {ROW_DTYPE.itemsize}]")
        rows = rows.contiguous().numpy().copy().view(ROW_DTYPE).reshape(-1)
    return Snapshot(blob, header, market_params=rows)


def save_snapshot(path, snap):
    torch.save(snapshot_record(snap), path)


def load_snapshot(path):
    """a snapshot file -> Snapshot with its blob on the CPU (validated; no device needed).  CDAVecEnv.restore moves it to the env's device."""
    return check_snapshot_record(torch.load(path, map_location="cpu", weights_only=True))
