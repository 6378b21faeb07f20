"""Batch WAL commit (Wal.append_commit_many → _native.wal_append_commit) against
the append ×N + commit path it replaces on the fused ingest path, the two
CRC-32 implementations against zlib, and a sanitizer run of the Python-free
WAL core."""

import os
import shutil
import struct
import subprocess
import threading
import zlib

import numpy as np
import pytest
import torch  # noqa: F401  (loads libc10 before the extension)

from greptimedb_amd import _native
from greptimedb_amd.engine.engine import EngineConfig, MitoEngine
from greptimedb_amd.engine.ingest import Ingestor
from greptimedb_amd.engine.wal import Wal
from greptimedb_amd.models.tsbs import CpuWorkload
from greptimedb_amd.query.executor import Executor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------- CRC

_IMPLS = ["table", "clmul"]
_BIG = 300_001
_RNG = np.random.RandomState(20261021)
_FILLS = {
    "random": _RNG.randint(0, 256, _BIG + 16).astype(np.uint8).tobytes(),
    "zeros": b"\x00" * (_BIG + 16),
    "ones": b"\xff" * (_BIG + 16),
}


def _need(impl):
    if impl == "clmul" and not _native.crc32_have_clmul():
        pytest.skip("CPU without pclmul + sse4.1")


@pytest.mark.parametrize("fill", sorted(_FILLS))
@pytest.mark.parametrize("impl", _IMPLS)
def test_crc32_matches_zlib(impl, fill):
    _need(impl)
    buf = _FILLS[fill]
    for n in list(range(0, 301)) + [4095, 4096, 4097, _BIG]:
        data = buf[:n]
        assert _native.crc32(data, 0, impl) == zlib.crc32(data), (impl, fill, n)
        assert _native.crc32(data, impl=impl) == zlib.crc32(data)
    # start offsets 0..15 into a larger buffer (a view, not a copy)
    view = memoryview(buf)
    for off in range(16):
        for n in (77, 1000, 4096):
            assert _native.crc32(view[off:off + n], 0, impl) == \
                zlib.crc32(view[off:off + n]), (impl, fill, off, n)
    # non-zero init, and chaining
    for init in (1, 0xDEADBEEF, 0xFFFFFFFF):
        for n in (0, 5, 64, 300, 4097, _BIG):
            assert _native.crc32(buf[:n], init, impl) == zlib.crc32(buf[:n], init)
    a = _native.crc32(buf[:1234], 0, impl)
    assert _native.crc32(buf[1234:5000], a, impl) == zlib.crc32(buf[:5000])


def test_crc32_auto_and_errors():
    buf = _FILLS["random"][:5000]
    assert _native.crc32(buf) == zlib.crc32(buf)
    assert _native.crc32(np.frombuffer(buf, dtype=np.uint8)) == zlib.crc32(buf)
    with pytest.raises(ValueError):
        _native.crc32(buf, 0, "nope")
    if not _native.crc32_have_clmul():
        with pytest.raises(RuntimeError):
            _native.crc32(buf, 0, "clmul")


# ------------------------------------------------------------ ingest runs

N_BATCHES, ROWS = 20, 300


def _engine(path, **kw):
    kw.setdefault("wal_shards", 4)
    return MitoEngine(EngineConfig(data_dir=str(path), device="cpu",
                                   background_flush=False, **kw))


def _ingestor(eng, wal_batch):
    ing = Ingestor(eng, default_regions=4)
    ing._bulk = True      # K16 bulk + fused path on CPU (cpu_ref kernels)
    ing._wal_batch = wal_batch
    return ing


def _batches(n=N_BATCHES, rows=ROWS, seed=5, tag=None):
    w = CpuWorkload(scale=23, seed=seed)
    if tag is not None:
        w.tagsets = [t.replace(b"host_", b"host_%d_" % tag) for t in w.tagsets]
    return [w.next_batch(rows) for _ in range(n)]


def _wal_files(eng_dir):
    d = os.path.join(str(eng_dir), "wal")
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def _frames(blob):
    """Independent frame walk: [(region, seq, payload)], all bytes consumed,
    every checksum verified with zlib."""
    out, off = [], 0
    while off < len(blob):
        body_len, crc = struct.unpack_from("<II", blob, off)
        body = blob[off + 8: off + 8 + body_len]
        assert len(body) == body_len >= 16
        assert zlib.crc32(body) == crc
        region, seq = struct.unpack_from("<QQ", body, 0)
        out.append((region, seq, body[16:]))
        off += 8 + body_len
    assert off == len(blob)
    return out


_SQL = ("SELECT hostname, count(*), min(usage_user), max(usage_user), "
        "min(usage_idle), max(usage_idle) FROM cpu GROUP BY hostname "
        "ORDER BY hostname")


def _query(eng):
    r = Executor(eng).execute(_SQL)
    return [list(c) for c in r.columns]


@pytest.fixture(scope="module")
def on_off(tmp_path_factory):
    """The same 20 batches through one thread with _wal_batch on and off."""
    base = tmp_path_factory.mktemp("on_off")
    batches = _batches()
    out = {}
    for name, wal_batch in [("on", True), ("off", False)]:
        eng = _engine(base / name)
        ing = _ingestor(eng, wal_batch)
        fused, commits = [], []
        orig_w, orig_c = eng.write_regions_fused, eng.commit_wal
        eng.write_regions_fused = lambda *a, _o=orig_w, **kw: (fused.append(kw.get("wal_batch")), _o(*a, **kw))[1]
        eng.commit_wal = lambda _o=orig_c: (commits.append(1), _o())[1]
        for b in batches:
            assert ing.ingest_lines(b) == ROWS
        del eng.commit_wal
        rows = _query(eng)
        eng.close()
        out[name] = {"dir": base / name, "fused": fused, "commits": commits,
                     "rows": rows, "files": _wal_files(base / name)}
    return out


def test_batch_path_is_taken(on_off):
    # the first batch registers the series on the general path
    assert on_off["on"]["fused"] == [True] * (N_BATCHES - 1)
    assert on_off["off"]["fused"] == [False] * (N_BATCHES - 1)
    # batched: commit_wal only for the general-path batch; off: every batch
    assert len(on_off["on"]["commits"]) == 1
    assert len(on_off["off"]["commits"]) == N_BATCHES


def test_wal_files_byte_identical(on_off):
    a, b = on_off["on"]["files"], on_off["off"]["files"]
    assert sorted(a) == sorted(b) and len(a) == 4
    for name in a:
        assert a[name] == b[name], name
    assert sum(len(v) for v in a.values()) > N_BATCHES * ROWS * 8 * 10


def test_replay_after_batch_run(on_off):
    want = sorted(f for blob in on_off["off"]["files"].values()
                  for f in _frames(blob))
    wal = Wal(str(on_off["on"]["dir"] / "wal"), shards=4)
    got = [(region, seq, payload) for _, region, seq, payload in wal.replay()]
    wal.close()
    assert len(got) == len(want) > 0
    assert [g[1] for g in got] == sorted(g[1] for g in got)   # seq order
    assert len({(g[0], g[1]) for g in got}) == len(got)       # each once
    assert sorted(got) == want
    assert on_off["on"]["rows"] == on_off["off"]["rows"]
    for name in ("on", "off"):
        eng = _engine(on_off[name]["dir"])
        assert _query(eng) == on_off["on"]["rows"]
        assert sum(_query(eng)[1]) == N_BATCHES * ROWS
        eng.close()


def test_rotation_and_purge(tmp_path):
    batches = _batches(n=40)
    files = {}
    for name, wal_batch in [("on", True), ("off", False)]:
        eng = _engine(tmp_path / name, wal_segment_bytes=64 << 10)
        ing = _ingestor(eng, wal_batch)
        for b in batches:
            ing.ingest_lines(b)
        eng.close()
        files[name] = _wal_files(tmp_path / name)
    assert files["on"] == files["off"]
    wal = Wal(str(tmp_path / "on" / "wal"), segment_bytes=64 << 10, shards=4)
    for sh in range(4):
        assert len(wal.segments(sh)) >= 3, wal.segments(sh)
    replayed = list(wal.replay())
    seqs = [seq for _, _, seq, _ in replayed]
    assert seqs == list(range(1, len(seqs) + 1))
    assert len(seqs) == sum(len(_frames(b)) for b in files["off"].values())
    assert len(seqs) >= 4 * 39    # one frame per region per fused batch
    # whole segments go, nothing at or above the cut is lost
    cut = seqs[len(seqs) // 2]
    before = set(wal.segments())
    wal.purge_before(cut)
    after = set(wal.segments())
    assert after < before
    kept = [seq for _, _, seq, _ in wal.replay()]
    assert set(s for s in seqs if s >= cut) <= set(kept)
    wal.close()
    # reopening restores every row
    eng = _engine(tmp_path / "off", wal_segment_bytes=64 << 10)
    assert sum(_query(eng)[1]) == 40 * ROWS
    eng.close()


def test_append_then_append_commit_many_keeps_order(tmp_path):
    wal = Wal(str(tmp_path / "wal"), shards=4)
    s1 = wal.append(8, b"buffered, not committed")
    payload = np.frombuffer(b"written through" * 50, dtype=np.uint8)
    s2, s3, s4 = wal.append_commit_many([8, 9, 12], [payload, b"", b"other"])
    assert (s1, s2, s3, s4) == (1, 2, 3, 4)
    assert wal.region_last == {8: 2, 9: 3, 12: 4}
    assert wal.append_commit_many([], []) == []
    # on disk already, before any commit(): shard 0 holds regions 8 and 12
    blob = open(os.path.join(wal.dir, wal.segments(0)[0]), "rb").read()
    assert _frames(blob) == [(8, 1, b"buffered, not committed"),
                             (8, 2, payload.tobytes()), (12, 4, b"other")]
    wal.commit()
    wal.close()
    wal = Wal(str(tmp_path / "wal"), shards=4)
    assert [(r, s) for _, r, s, _ in wal.replay()] == [(8, 1), (8, 2), (9, 3), (12, 4)]
    assert wal.next_seq == 5
    wal.close()


def test_wal_append_commit_errors_leave_writers_usable(tmp_path):
    w = _native.WalWriter()
    with pytest.raises(RuntimeError):      # no open segment
        _native.wal_append_commit([w], [1], [1], [b"x"], False)
    with pytest.raises(RuntimeError):      # lengths differ
        _native.wal_append_commit([w], [1, 2], [1], [b"x"], False)
    with pytest.raises(Exception):         # not a buffer
        _native.wal_append_commit([w], [1], [1], [object()], False)
    w.open_segment(str(tmp_path / "a.wal"))
    sizes = _native.wal_append_commit([w, w], [1, 1], [1, 2], [b"x", b"yz"], True)
    assert sizes == [25, 51] and w.segment_bytes() == 51
    w.rotate(str(tmp_path / "b.wal"))
    assert _native.wal_append_commit([w], [1], [3], [b""], False) == [24]
    w.close_segment()
    assert [(r, s, p) for r, s, p in _native.wal_read_segment(str(tmp_path / "a.wal"))] == \
        [(1, 1, b"x"), (1, 2, b"yz")]
    assert _native.wal_read_segment(str(tmp_path / "b.wal")) == [(1, 3, b"")]


def test_six_threads_batch_commit(tmp_path):
    n_threads, n_batches = 6, 100
    eng = _engine(tmp_path / "e", wal_segment_bytes=1 << 20)
    work = [(_ingestor(eng, True), _batches(n=10, seed=11 + t, tag=t))
            for t in range(n_threads)]
    errors = []

    def run(ing, batches):
        try:
            for k in range(n_batches):
                assert ing.ingest_lines(batches[k % len(batches)]) == ROWS
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=run, args=w) for w in work]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    total = n_threads * n_batches * ROWS
    assert sum(_query(eng)[1]) == total
    eng.close()
    files = _wal_files(tmp_path / "e")
    assert len(files) > 4    # rotated while six threads were writing
    frames = [f for blob in files.values() for f in _frames(blob)]  # CRCs
    seqs = sorted(seq for _, seq, _ in frames)
    assert seqs == list(range(1, len(seqs) + 1))    # unique and gap-free
    eng = _engine(tmp_path / "e", wal_segment_bytes=1 << 20)
    assert sum(_query(eng)[1]) == total
    eng.close()


def test_wal_sync_path(tmp_path):
    batches = _batches(n=4)
    eng = _engine(tmp_path / "e", wal_sync=True)
    assert eng.wal.sync_on_commit
    ing = _ingestor(eng, True)
    for b in batches:
        ing.ingest_lines(b)
    eng.close()
    eng = _engine(tmp_path / "e")
    assert sum(_query(eng)[1]) == 4 * ROWS
    eng.close()


def test_sync_covers_every_acknowledged_frame(tmp_path):
    """wal_sync with ONE shard: a batch's frames share a writer and only the
    last carries the sync. Nothing acknowledged may stay unsynced, across a
    rotation and when a write-through call flushed somebody's buffered frame."""
    wal = Wal(str(tmp_path / "wal"), segment_bytes=4096, sync_on_commit=True,
              shards=1)
    w = wal.shards[0].writer
    payload = b"p" * 700
    for _ in range(12):     # rotates every other batch
        wal.append_commit_many([1, 2, 3, 4], [payload] * 4)
        assert w.unsynced_bytes() == 0
    assert len(wal.segments(0)) >= 5
    syncs = w.sync_count()
    assert syncs >= 12
    # general path: append, then someone's batch flushes it, then commit()
    wal.append(9, b"buffered")
    _native.wal_append_commit([w, w], [1, 2], [900, 901], [b"a", b"b"], False)
    assert w.unsynced_bytes() > 0
    wal.commit()            # its buffer is empty by now; it must sync anyway
    assert w.unsynced_bytes() == 0 and w.sync_count() == syncs + 1
    # rotation between the frames of a batch: old segment synced before close
    _native.wal_append_commit([w], [1], [902], [b"first frames"], False)
    w.rotate(str(tmp_path / "wal" / f"{903:020d}.wal"), True)
    assert w.unsynced_bytes() == 0 and w.sync_count() == syncs + 2
    _native.wal_append_commit([w], [1], [903], [b"last frame"], True)
    assert w.unsynced_bytes() == 0 and w.sync_count() == syncs + 3
    wal.close()


# ----------------------------------------- sanitizer runs of the WAL core

@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_wal_core_under_host_sanitizers(tmp_path, sanitize):
    """Build csrc/wal_core_check.cpp (a stand-alone program over the frame,
    CRC and writer core) with the host compiler and run it."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "wal_core_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=" + sanitize, "-pthread",
           os.path.join(ROOT, "csrc", "wal_core_check.cpp"), "-o", exe]
    if sanitize != "thread":
        cmd.insert(6, "-fno-sanitize-recover=undefined")
    # sanitizer runtimes linked into the program itself where the compiler
    # offers it (gcc), so the run does not depend on library load order
    static_flags = ["-static-libtsan"] if sanitize == "thread" else \
        ["-static-libasan", "-static-libubsan"]
    static = subprocess.run(cmd + static_flags, capture_output=True, text=True)
    if static.returncode != 0:
        subprocess.run(cmd, check=True)
    scratch = tmp_path / "segments"
    scratch.mkdir()
    r = subprocess.run([exe, str(scratch)], capture_output=True, text=True)
    # Not a finding: the TSan runtime of some compilers cannot place its
    # shadow memory under a kernel with high-entropy address randomisation
    # and exits before main. Run that process without randomisation instead.
    no_map = "ThreadSanitizer: unexpected memory mapping"
    if no_map in r.stderr and shutil.which("setarch"):
        r = subprocess.run(["setarch", os.uname().machine, "-R", exe, str(scratch)],
                           capture_output=True, text=True)
    if no_map in r.stderr:
        pytest.skip("the TSan runtime cannot map its shadow memory here")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "wal_core_check ok" in r.stdout
