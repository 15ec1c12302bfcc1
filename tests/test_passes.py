"""The pass runner without a GPU (gencore_amd/csrc/gce_passes.hpp, gce_run_bam_passes): the --device_memory rules of the command line on both
sides of each, and the Python statement of the plan (gencore_amd/shard.py: weighted_cuts, pass_watermarks) on hand-made keys.  The GPU suite
(test_passes_gpu.py) compares that statement with the C planner."""
import numpy as np
import pytest

from test_cli import cli


@pytest.fixture
def workdir(tmp_path):
    (tmp_path / "in.bam").write_bytes(b"")
    return tmp_path


BAD_MEMORY = ["0", "-1", "abc", "nan", "inf", ""]


@pytest.mark.parametrize("value", BAD_MEMORY)
def test_device_memory_rejected(workdir, value):
    r = cli(["-i", "in.bam", "-r", "ref.fa", "--device_memory", value], workdir)
    assert r.returncode != 0 and r.stdout == ""
    assert r.stderr == "ERROR: device_memory should be a positive number of GB or auto, got '%s'\n" % value
    assert not (workdir / "gencore.json").exists()


@pytest.mark.parametrize("value", ["auto", "0.001", "2", "192.5"])
def test_device_memory_accepted(workdir, value):
    """An accepted value passes its rule: the run goes on to the coverage step this command checks before it (and fails there)."""
    r = cli(["-i", "in.bam", "-r", "ref.fa", "--coverage_sampling", "0", "--device_memory", value], workdir)
    assert r.returncode != 0 and r.stderr == "ERROR: coverage_sampling should be greater than 0\n"
    r = cli(["-i", "in.bam", "-r", "ref.fa", "--level", "7", "--devices", "0", "--coverage_sampling", "-1", "--device_memory", value], workdir)
    assert r.stderr == "ERROR: coverage_sampling should be greater than 0\n"


def test_device_memory_one_device_only(workdir):
    r = cli(["-i", "in.bam", "-r", "ref.fa", "--devices", "0,1", "--device_memory", "4"], workdir)
    assert r.returncode != 0 and r.stderr == "ERROR: device_memory works on one device; it cannot be combined with several --devices\n"
    # auto (the default) with several devices is the sharded runner as before: validation passes, the run fails later on the empty file
    r = cli(["-i", "in.bam", "-r", "ref.fa", "--devices", "0,1", "--device_memory", "auto", "--coverage_sampling", "0"], workdir)
    assert r.stderr == "ERROR: coverage_sampling should be greater than 0\n"


def test_help_names_device_memory(workdir):
    r = cli(["--help"], workdir)
    assert r.returncode == 0 and "--device_memory" in r.stdout


def brute_cuts(key, weight, world):
    """weighted_cuts by enumeration: cut r = smallest key k such that the weight of keys <= k exceeds total * r / world."""
    total = int(np.sum(weight))
    uk = np.unique(key)
    w_le = np.asarray([int(weight[key <= k].sum()) for k in uk])
    cuts = []
    for r in range(1, world):
        ok = uk[w_le * world > total * r]
        cuts.append(int(ok[0]) if len(ok) else int(uk[-1]))
    return cuts


@pytest.mark.parametrize("seed", range(6))
def test_weighted_cuts(seed):
    from gencore_amd.shard import weighted_cuts
    rng = np.random.RandomState(seed)
    n = int(rng.randint(1, 400))
    key = ((rng.randint(0, 3, n).astype(np.uint64) << np.uint64(32)) | rng.randint(0, 50, n).astype(np.uint64))
    weight = rng.randint(1, 5000, n).astype(np.uint64)
    for world in (1, 2, 3, 7, 64):
        cuts = weighted_cuts(key, weight, world)
        assert len(cuts) == world - 1
        assert [int(c) for c in cuts] == brute_cuts(key, weight, world)
        rng_of = np.searchsorted(cuts, key, side="right")
        for k in np.unique(key):                                     # every key in one range
            assert len(set(rng_of[key == k].tolist())) == 1
        assert np.all(np.diff(np.asarray(cuts, np.uint64).astype(np.float64)) >= 0)
        # a range weighs at most its share plus one key
        heavy = max(int(weight[key == k].sum()) for k in np.unique(key))
        for r in range(world):
            assert int(weight[rng_of == r].sum()) <= int(weight.sum()) // world + heavy + 1


def test_weighted_cuts_balance_by_weight_not_count():
    """Ten light reads on key 1 and one heavy read on key 2: halving by weight puts the cut on key 2, halving by count on key 1."""
    from gencore_amd.shard import weighted_cuts
    key = np.asarray([1] * 10 + [2], np.uint64)
    assert int(weighted_cuts(key, np.asarray([1] * 10 + [100], np.uint64), 2)[0]) == 2
    assert int(weighted_cuts(key, np.asarray([100] * 10 + [1], np.uint64), 2)[0]) == 1
    assert list(weighted_cuts(np.zeros(0, np.uint64), np.zeros(0, np.uint64), 3)) == [2 ** 64 - 1] * 2


def core_of(rows):
    from gencore_amd.capi import CORE_DTYPE
    c = np.zeros(len(rows), CORE_DTYPE)
    for i, (tid, pos, mtid, mpos, isize) in enumerate(rows):
        c[i]["tid"], c[i]["pos"], c[i]["mtid"], c[i]["mpos"], c[i]["isize"] = tid, pos, mtid, mpos, isize
        c[i]["l_qname"], c[i]["n_cigar"], c[i]["l_qseq"] = 10, 1, 100
    return c


def test_watermark_from_the_reads():
    """W_k is the smallest (tid, pos) of the reads of later ranges -- not their key: the right mate of a near pair has its key at the
    mate's position, and a read whose isize sign disagrees with the positions keys on its own position; unmapped reads emit nothing."""
    from gencore_amd.shard import cluster_key, pass_watermarks
    core = core_of([(0, 100, 0, 300, 300), (0, 300, 0, 100, -300),          # a near pair: both keyed at 100
                    (0, 200, 0, 400, 300), (0, 400, 0, 200, -300),          # keyed at 200
                    (0, 250, 0, 150, 100),                                  # isize > 0 though the mate lies in front: keyed at 250
                    (1, 10, 1, 20, 10), (-1, -1, -1, -1, 0)])               # contig 1; an unmapped read (key last)
    key = cluster_key(core)
    assert list(key[:5]) == [100, 100, 200, 200, 250]
    shard = np.searchsorted(np.asarray([200, 250, 1 << 32]), key, side="right")
    assert list(shard) == [0, 0, 1, 1, 2, 3, 3]
    wm = pass_watermarks(core, shard, 4)
    assert wm[0] == (0, 200)                    # the smallest read of ranges 1..3; range 0's right mate at 300 lies behind it: it is held
    assert wm[1] == (0, 250)
    assert wm[2] == (1, 10)                     # the unmapped read of range 3 (tid -1, never written) holds nothing back
    assert wm[3] == (2 ** 31 - 1, 2 ** 31 - 1)
    only_unmapped = np.where(np.arange(len(core)) == 6, 3, np.minimum(shard, 2))
    assert pass_watermarks(core, only_unmapped, 4)[2] == (2 ** 31 - 1, 2 ** 31 - 1)       # a later range of unmapped reads only: nothing held


def test_plan_shards_weight_mode_spec():
    """plan_shards(mode="weight") is weighted_cuts over pass_weights: whole keys per range, ranges in key order."""
    from gencore_amd.shard import cluster_key, pass_weights, plan_shards, weighted_cuts
    rng = np.random.RandomState(5)
    rows = [(int(t), int(p), int(t), int(p) + 200, 200) for t, p in zip(rng.randint(0, 2, 300), rng.randint(0, 5000, 300))]
    core = core_of(rows)
    core["l_qseq"] = rng.randint(50, 300, len(core))
    sh = plan_shards(core, 5, mode="weight")
    key = cluster_key(core)
    order = np.argsort(key, kind="stable")
    assert np.all(np.diff(sh[order]) >= 0)
    w = pass_weights(core)
    assert int(w[0]) == 6 * (36 + 10 + 4 + (int(core["l_qseq"][0]) + 1) // 2 + int(core["l_qseq"][0])) + 1024
    assert list(sh) == list(np.searchsorted(weighted_cuts(key.astype(np.uint64), w, 5), key.astype(np.uint64), side="right"))
