"""Measurement tooling (CPU): the PMC summary's kernel families (tools/pmc_traffic.py) name
each traced kernel as bench.py's roofline expects, so a profile attributes its counters to
the right launch."""
import importlib.util
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _pmc():
    spec = importlib.util.spec_from_file_location("pmc_traffic", os.path.join(HERE, "..", "tools", "pmc_traffic.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_kernel_families():
    fam = _pmc().family
    ns = "(anonymous namespace)::"
    args = "((anonymous namespace)::DevGraph, (anonymous namespace)::FRec const*)"
    assert fam(f"void {ns}bidi_kernel<16, 9, 128, 64, 7, 1, 0>{args}") == "bidi_kernel<16>"
    assert fam(f"void {ns}bidi_kernel<16, 9, 128, 64, 7, 1, 1>{args}") == "bidi_kernel<16> (pipelined chunks)"
    assert fam(f"{ns}bidi_host_kernel<2>{args}") == "bidi_host_kernel (host batches)"
    assert fam(f"void {ns}bidi_kernel<16, 11, 384, 256, 6, 1, 0>{args}") == "bidi spill stage w (16 requests, 2048 slots)"
    assert fam(f"void {ns}bidi_kernel<1, 13, 1024, 256, 7, 1, 0>{args}") == "bidi single-request stage"
    assert fam(f"void {ns}unit2_kernel<16>{args}") == "unit2_kernel<16>"
    assert fam(f"{ns}part_apply_kernel({ns}PartDev)") == "part_apply_kernel"
    assert fam(f"{ns}part_gather_kernel({ns}PartDev, unsigned long, unsigned long)") == "part_gather_kernel"
    assert fam(f"{ns}clear_kernel(unsigned long*)") is None


def test_label_kernel_families():
    """plan label's kernels and the two-tier label path's (round 5): tier_label_kernel is its
    own family, not label_kernel's"""
    fam = _pmc().family
    ns = "(anonymous namespace)::"
    assert fam(f"void {ns}label_kernel<32, 32>({ns}LabelGraph, unsigned int const*)") == "label_kernel"
    assert fam(f"void {ns}label_full_kernel<32, 32>({ns}LabelGraph)") == "label_full_kernel (overflow lists)"
    assert fam(f"void {ns}label_host_kernel<32, 32>(DevGraph)") == "label_host_kernel (host batches)"
    assert fam(f"void {ns}tier_label_kernel<false>(ketogpu::tier::Graph)") == "tier_label_kernel"
    assert fam(f"{ns}tier_label_reply_kernel(ketogpu::tier::Graph)") == \
        "tier_label exchange kernels (pairs, replies, lengths, bounds)"
    assert fam(f"{ns}tier_pair_kernel(ketogpu::tier::Graph)") == \
        "tier_label exchange kernels (pairs, replies, lengths, bounds)"
    assert fam(f"{ns}tier_reply_len_kernel(ketogpu::tier::Graph)") == "tier_reply kernels (len + scan + copy)"


def test_partitioned_r2_sample_flags_mismatches():
    """bench.py --r2-sample: the independent R2 checker fed from the config #5 row stream agrees
    with the oracle's answers, and a flipped answer is reported"""
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(HERE, ".."))
    import bench
    from keto_amd import synth
    from oracle import oracle as O
    w = synth.config5(users=30000, groups=3000, docs=6000, tuples=150000, checks=3000, seed=17)
    st = O.Store(w.namespaces, 100)
    for cols in w.batches(4093):
        st.add_columnar(cols)
    want = st.finalize(presorted=True).check_batch(w.requests(range(w.n_checks)), nthreads=4).astype(bool)
    ok = bench.r2_stream(w, want, 1000)
    assert ok["sample"] == 1000 and ok["mismatches"] == 0
    bad = want.copy()
    bad[:40] ^= True
    assert bench.r2_stream(w, bad, 3000)["mismatches"] == 40


SMALL = dict(users=3000, groups=300, docs=600, tuples=15000, checks=1000)


def test_bench_input_cache_round_trip(tmp_path):
    """bench.py's plain run: the snapshot and the resolved requests read back from the cache
    files are the ones the generator and the builder made; a run that needs the rows
    (--full) neither reads nor writes the files"""
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(HERE, ".."))
    import bench
    cache = str(tmp_path / "cache")
    w, snap, roots, targets, t = bench.load_inputs(SMALL, "unit", cache, need_workload=False)
    assert w is not None and t["cache_load"] is None and len(os.listdir(cache)) == 2
    w2, snap2, roots2, targets2, t2 = bench.load_inputs(SMALL, "unit", cache, need_workload=False)
    assert w2 is None and t2["cache_load"] is not None
    np.testing.assert_array_equal(roots2, roots)
    np.testing.assert_array_equal(targets2, targets)
    g, g2 = snap.graph(), snap2.graph()
    for k in g:
        np.testing.assert_array_equal(g2[k], g[k])
    assert snap2.stats() == snap.stats()
    # other sizes: other files; --full: the generator, whatever the cache holds
    w3, _, roots3, _, t3 = bench.load_inputs(dict(SMALL, checks=500), "unit", cache, need_workload=False)
    assert w3 is not None and len(roots3) == 500 and len(os.listdir(cache)) == 4
    w4, _, roots4, _, t4 = bench.load_inputs(SMALL, "unit", cache, need_workload=True)
    assert w4 is not None and t4["cache_load"] is None and len(os.listdir(cache)) == 4
    np.testing.assert_array_equal(roots4, roots)


def test_bench_input_cache_drops_stale_files(tmp_path):
    """writing the cache removes the finished files of the same workload made at other
    sources, and nothing else: not another run's temporary file, not another workload"""
    import sys
    sys.path.insert(0, os.path.join(HERE, ".."))
    import bench
    cache = tmp_path / "cache"
    cache.mkdir()
    stale = ["unit_c1000_0123456789abcdef.snap", "unit_c1000_0123456789abcdef.ids.npz"]
    kept = ["unit_c1000_0123456789abcdef.4242.tmp", "unit_c500_0123456789abcdef.snap", "other_c1000_00.snap"]
    for f in stale + kept:
        (cache / f).write_bytes(b"x")
    bench.load_inputs(SMALL, "unit", str(cache), need_workload=False)
    left = set(os.listdir(cache))
    assert not left & set(stale) and set(kept) <= left and len(left) == len(kept) + 2
    assert bench.load_inputs(SMALL, "unit", str(cache), need_workload=False)[0] is None  # read back
    assert set(os.listdir(cache)) == left


@pytest.mark.gpu
def test_bench_plain_run_line_and_dump(tmp_path):
    """`bench.py --small --steps 3 --warmup 1 --dump-outputs DIR`: a plain run prints the line
    with the headline fields and no --full leg, and DIR/allowed.npy holds the last timed
    step's answers (float32), equal to ketogpu_check_ids over the same requests"""
    import json
    import subprocess
    import sys
    import numpy as np
    from keto_amd import check
    from keto_amd.snapshot import Snapshot
    root = os.path.join(HERE, "..")
    cache, dump = str(tmp_path / "cache"), str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--small", "--cache-dir", cache, "--dump-outputs", dump], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["unit"] == "checks/s" and d["higher_is_better"] is True and d["steps"] == 3 and d["warmup"] == 1
    assert d["full"] is False and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 100_000) < 0.01 * 100_000  # value = requests / step time
    for k in ("roofline", "cpu_baseline", "parity", "host_to_host_checks_per_s", "resident_call_checks_per_s"):
        assert k not in d
    got = np.load(os.path.join(dump, "allowed.npy"))
    assert got.dtype == np.float32 and got.shape == (100_000,)
    assert set(np.unique(got)) <= {0.0, 1.0}
    # the CPU oracle over the same workload, generated here: a seeded sample of 5000 of
    # the requests (the oracle's DFS takes 20 s for all of them), entry for entry
    sys.path.insert(0, root)
    import bench
    from tests import randgraph
    name, _, sizes = bench.config2_sizes(True, 1)
    w, _, roots, targets, _ = bench.load_inputs(sizes, name, "", need_workload=True)
    idx = np.sort(np.random.default_rng(0).choice(w.n_checks, 5000, replace=False))
    want = randgraph.oracle_store_columns(w.namespaces, w.columns).check_batch(w.requests(idx), nthreads=8)
    assert 0.4 < want.mean() < 1.0  # half the requests are constructed positives
    np.testing.assert_array_equal(got[idx], np.asarray(want, dtype=np.float32))
    # and every entry against the host-to-host call over the cached snapshot and ids
    snap_file = [f for f in os.listdir(cache) if f.endswith(".snap")][0]
    snap = Snapshot.load(os.path.join(cache, snap_file))
    with np.load(os.path.join(cache, snap_file[:-5] + ".ids.npz")) as z:
        np.testing.assert_array_equal(z["roots"], roots)
        np.testing.assert_array_equal(z["targets"], targets)
        np.testing.assert_array_equal(got, check.Engine(snap).check_ids(z["roots"], z["targets"]).astype(np.float32))


def test_synth_rbac_output_pinned():
    """the config #2 generator's rows, offsets and checks, byte for byte: the hash was taken
    from the serial generator, before its rows were emitted on several threads"""
    import hashlib
    import numpy as np
    from keto_amd import synth
    w = synth.rbac(10_000, 100, 2_000, 50_000, 1_000, seed=synth.SEED, check_seed=synth.SEED + 1)
    assert w.counts == {"parent": 149, "member": 29946, "grant": 19905, "tuples": 50000}
    h = hashlib.sha256()
    for k in sorted(w.columns):
        if w.columns[k] is not None:
            h.update(k.encode())
            h.update(np.ascontiguousarray(w.columns[k]).tobytes())
    for a in (w.chk_doc, w.chk_user, w.chk_pos):
        h.update(a.tobytes())
    assert h.hexdigest()[:20] == "ca465ddd3c06a4065d16"


def test_bench_last_step_copy():
    """the dump reads the copy the last timed step ran on (step k: copy k mod PIPE_COPIES)"""
    import sys
    sys.path.insert(0, os.path.join(HERE, ".."))
    import bench
    assert [bench.last_step_copy(s, 2) for s in (1, 2, 3, 20, 2001)] == [0, 1, 0, 1, 0]
    assert [bench.last_step_copy(s, 3) for s in (1, 3, 4)] == [0, 2, 0]
    assert bench.PIPE_COPIES >= 1
