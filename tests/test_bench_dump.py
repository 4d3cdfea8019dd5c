"""CPU: bench.py --dump-outputs (the last timed step's per-read results and PAF
text as float arrays, in read order, capped by a fixed seeded sample) and the
--full switch's default."""
import ctypes as C

import numpy as np

import bench
from minimap2_rs_amd import _lib as L


def _unit(k, lo, n, text):
    res = (L.ReadResult * n)()
    for i in range(n):
        res[i].flags, res[i].score, res[i].sum_k, res[i].dv = 1, lo + i, (1 << 40) + lo + i, 0.125 * (i + 1)
    return {"k": k, "n": n, "res": res, "buf": C.create_string_buffer(text + b"garbage past len"), "len": len(text)}


def test_plain_run_is_the_default():
    a = bench.parse([])
    assert not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_in_read_order(tmp_path):
    us = [_unit(1, 3, 2, b"r3\tx\nr4\ty\n"), _unit(0, 0, 3, b"r0\ta\nr2\tb\n")]     # shares out of order
    d = tmp_path / "out"
    bench.dump_outputs(str(d), 0, us)
    res = np.load(d / "results.npy")
    assert res.dtype == np.float64 and res.shape == (5, len(bench.RES_DTYPE.names))
    col = {f: res[:, i] for i, f in enumerate(bench.RES_DTYPE.names)}
    assert col["score"].tolist() == [0, 1, 2, 3, 4] and col["sum_k"].tolist() == [(1 << 40) + i for i in range(5)]
    assert col["dv"].tolist() == [0.125, 0.25, 0.375, 0.125, 0.25]
    paf = np.load(d / "paf_bytes.npy")
    assert paf.dtype == np.float32 and bytes(paf.astype(np.uint8)) == b"r0\ta\nr2\tb\nr3\tx\nr4\ty\n"
    bench.dump_outputs(str(d), 2, us)
    assert (d / "results_rank2.npy").exists() and (d / "paf_bytes_rank2.npy").exists()


def test_dump_sample_is_fixed_and_within_budget():
    res = np.zeros(1000, dtype=bench.RES_DTYPE)
    res["score"] = np.arange(1000)
    paf = b"".join(b"read%d\t%s\n" % (i, b"x" * (i % 50)) for i in range(1000))
    budget = 16384
    a = bench.dump_arrays(res, paf, budget)
    b = bench.dump_arrays(res, paf, budget)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.nbytes for v in a.values()) <= budget
    score = a["results"][:, bench.RES_DTYPE.names.index("score")]
    assert 0 < len(score) < 1000 and np.all(np.diff(score) > 0)
    kept = bytes(a["paf_bytes"].astype(np.uint8)).splitlines(keepends=True)
    ids = [int(ln.split(b"\t")[0][4:]) for ln in kept]
    assert kept and set(kept) <= set(paf.splitlines(keepends=True)) and ids == sorted(ids)
    whole = bench.dump_arrays(res, paf)
    assert len(whole["results"]) == 1000 and len(whole["paf_bytes"]) == len(paf)
