"""CPU side of the output-table tests (tests/outcases.py): every case builds, the oracle returns status 0 on it, its premise -- facts about the batch and the
oracle's out_flag / mate / nm_new that put it into the catalogue -- holds, the catalogue is frozen by a digest of every batch, and the model table
(outcases.rows_from_table of the oracle's result: what the GPU test holds the engine's rows against) passes check_output_order and round-trips through
table_from_rows.  check_output_order itself is held against a table with two neighbours of a run swapped.  No GPU.

Measured on the CPU host the suite runs on (pytest -s prints the large case's): 63 streams, 4.68 M reads, the module's 130 tests 12 s; of that the large case
(4 198 405 reads) 7.3 s: 2.8 s to build it and run the oracle (0.4 s), 1.7 s for the model table, 2.0 s for check_output_order, 0.8 s for the round trip;
the 67-tile stream 1.3 s, every other case below 0.2 s."""
import hashlib
import time

import numpy as np
import pytest

import outcases as oc
from gencore_amd.batch import ReadBatch, table_from_rows
from parity_helpers import check_output_order, diff_results


def batch_digest(case):
    h = hashlib.sha256()
    for f in ReadBatch.FIELDS:
        a = getattr(case.batch, f)
        h.update(f.encode()); h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    h.update(repr((case.size_req, tuple(case.contig_len), case.contigs, case.group)).encode())
    return h.hexdigest()[:16]


FROZEN = {
    "size:1": "ee0569e18ec598ff",
    "size:1:fillers": "40f707a9697e8040",
    "size:7": "94436ddaac2c72b2",
    "size:7:fillers": "58555e7f4eabee3a",
    "size:8": "eb665a7bfafba791",
    "size:8:fillers": "371106b8477db280",
    "size:9": "ae7f8ea2d63d5287",
    "size:9:fillers": "786213b047fc541c",
    "size:63": "45556cb3ce7f2a92",
    "size:63:fillers": "cd957604be45a5f4",
    "size:64": "182b95e49d73a77e",
    "size:64:fillers": "14bc45c4b0cb3180",
    "size:65": "21878aef2a7db137",
    "size:65:fillers": "40d48323e0d806e8",
    "size:4095": "2b74f49005d1f06f",
    "size:4095:fillers": "9373e9a6e21c4497",
    "size:4096": "d495986f30df1998",
    "size:4096:fillers": "fc48ee4adc52d962",
    "size:4097": "5cfc859809f6d1a1",
    "size:4097:fillers": "fe7271d15a176d1f",
    "size:8191": "0f7a8988d8a2ccdc",
    "size:8191:fillers": "4bf1cf98a133ca01",
    "size:8193": "53eb4daf8617c5f7",
    "size:8193:fillers": "510582eaf5285d82",
    "tail:1": "9699c897988749b2",
    "tail:1:pair": "c86dea6b90a3ed35",
    "tail:2": "56fb70894db2fe61",
    "tail:2:pair": "50296f697920a75e",
    "tail:3": "8615eba70cc899b5",
    "tail:3:pair": "070b6463b1f93e32",
    "tail:4": "bb829048fab7ef9e",
    "tail:4:pair": "d20ac4fa4f8cee0a",
    "tail:5": "292ca716a33b382f",
    "tail:5:pair": "7f73cd480d18abc5",
    "tail:6": "b1dcce8049d087f5",
    "tail:6:pair": "1a0f703113cdf2d0",
    "tail:7": "22f1066765751ce4",
    "tail:7:pair": "01d420ca24f2b317",
    "len:0": "b2ad0e6b15f75065",
    "len:1": "efd685a7bc83412d",
    "len:2": "70d582436b01e2f7",
    "len:31": "1ed6198891522366",
    "len:32": "748cc03ab44b3aef",
    "len:33": "3bff5911e7e818ce",
    "len:255": "e88e0403b3168470",
    "len:256": "9e622de92e5c035d",
    "len:257": "447b23704bf979c2",
    "len:mixed": "8aef51cb15ebd5a7",
    "lq:dropped_other_length": "c7828c3736c6cdd7",
    "lq:pass_through_other_length": "63e2d4daba94c8a4",
    "lq:filtered_cluster_other_length": "8840f340ffa3aa16",
    "stats:67_tiles_mixed": "6bea2dc76cca822e",
    "stats:nm_patched": "ea0a33d128b5a126",
    "runs:300": "0d7acb53704e792a",
    "runs:5000": "3559815ba94c85f2",
    "runs:4000_4200": "1b3f1d75e82765cf",
    "runs:first_last": "cc812070b68dc599",
    "mates:places": "e893b9386cbaaf6c",
    "cap:1": "9b3e6267a3d10a5f",
    "cap:17": "0d52ce6ea27676b5",
    "cap:33": "4c889b688c73fee6",
    "cap:one_blob_33": "fd9dba43ad4846dd",
    "large:1025_tiles": "7dfa28377708b538",
}


def test_catalogue_holds_every_family():
    assert set(FROZEN) == set(oc.CASES)
    for g, fam in oc.GROUPS.items():
        assert oc.family(fam), fam
    assert (len(oc.family("size")), len(oc.family("tail")), len(oc.family("len")), len(oc.family("lq"))) == (2 * len(oc.SIZES), 14, len(oc.LENGTHS) + 1, 3)
    assert len(oc.CASES) == 63


@pytest.mark.parametrize("name", list(oc.CASES))
def test_case_builds_and_its_premise_holds(oracle, name):
    case = oc.get(name)
    assert case.batch.n > 0 and oc.GROUPS[case.group] in (name.split(":")[0], "len" if name.startswith("lq:") else "")
    assert batch_digest(case) == FROZEN[name], "%s drifted: %s" % (name, batch_digest(case))
    want = oc.oracle_result(name)
    assert want.status == 0, (name, want.status, want.message)
    prem = case.premise(want)
    bad = [k for k, v in prem.items() if not v]
    assert prem and not bad, "%s: premise does not hold: %s" % (name, bad)


@pytest.mark.parametrize("name", list(oc.CASES))
def test_model_table_is_ordered_and_round_trips(oracle, name):
    case, want = oc.get(name), oc.oracle_result(name)
    t0 = time.perf_counter()
    rows = oc.rows_from_table(case.batch, want)
    t1 = time.perf_counter()
    assert not check_output_order(case.batch, rows)
    t2 = time.perf_counter()
    back = table_from_rows(case.batch, rows, want.pre, want.post)
    assert not diff_results(case.batch, back, want)
    em = want.out_flag != 0                                                        # (what the oracle notes on a read it does not emit is not part of the table)
    assert np.array_equal(back.out_flag, want.out_flag)
    for f in ("qname_src", "nm_new", "fr", "rr", "mate"):
        assert np.array_equal(getattr(back, f)[em], getattr(want, f)[em]), f
    if case.batch.n > 1000000:
        print("\n%s: model table %.2f s, check_output_order %.2f s, round trip %.2f s" % (name, t1 - t0, t2 - t1, time.perf_counter() - t2))


def test_back_to_back_order_goes_down_and_up_and_flips_the_uniform_path():
    names = oc.back_to_back_order()
    assert sorted(names) == sorted(n for n in oc.CASES if not n.startswith("large:")) and len(names) == 62
    n = np.asarray([oc.get(x).batch.n for x in names])
    d = np.sign(np.diff(n))
    assert int((d[1:] * d[:-1] < 0).sum()) >= 50                                   # the size turns round at nearly every step
    uni = np.asarray([oc.uniform_length(oc.get(x).batch.core) >= 0 for x in names])
    assert int((uni[1:] != uni[:-1]).sum()) >= 8
    assert max(n) > 64 * oc.TILE and min(n) == 1


def test_check_output_order_rejects_a_swap_inside_a_run(oracle):
    """Two neighbouring rows of one (tid, pos) run that differ only in isize, only in mpos, only in mtid, or only in the input index, swapped: every one
    of them is a table out of order."""
    case, want = oc.get("runs:300"), oc.oracle_result("runs:300")
    rows = oc.rows_from_table(case.batch, want)
    assert not check_output_order(case.batch, rows)
    c = case.batch.core[rows["src"].astype(np.int64)]
    eq = {f: c[f][1:] == c[f][:-1] for f in ("tid", "pos", "mtid", "mpos", "isize")}
    run = eq["tid"] & eq["pos"]
    for only, sel in (("isize", run & eq["mtid"] & eq["mpos"] & ~eq["isize"]), ("mpos", run & eq["mtid"] & ~eq["mpos"] & eq["isize"]),
                      ("mtid", run & ~eq["mtid"]), ("index", run & eq["mtid"] & eq["mpos"] & eq["isize"])):
        at = np.nonzero(sel)[0]
        assert len(at), only
        k = int(at[len(at) // 2])
        swapped = {f: (v.copy() if f in ("src", "kind", "qname_src", "nm_new", "fr", "rr") else v) for f, v in rows.items()}
        for f in ("src", "kind", "qname_src", "nm_new", "fr", "rr"):
            swapped[f][[k, k + 1]] = rows[f][[k + 1, k]]
        assert check_output_order(case.batch, swapped) == ["rows are not in bamComp order"], only


def test_blob_contract_check_holds_on_the_model_and_rejects_overlap(oracle):
    """The header's contract for the blobs as the GPU test checks it (check_blobs): the model's own layout passes; two records on one interval, an offset off
    the 16-byte grid and a total that is not the sum of the units do not."""
    check_blobs = oc.check_blobs
    case, want = oc.get("len:mixed"), oc.oracle_result("len:mixed")
    rows = oc.rows_from_table(case.batch, want)
    assert not check_blobs(case.batch, rows)
    lq = case.batch.core["l_qseq"][rows["src"].astype(np.int64)]
    k = int(np.nonzero((lq[:-1] > 0) & (lq[1:] > 0))[0][0])
    for f, delta in (("seq_off", None), ("qual_off", None), ("seq_off", 8), ("qual_off", 8)):
        bad = dict(rows); bad[f] = rows[f].copy()
        bad[f][k + 1] = rows[f][k] if delta is None else rows[f][k + 1] + np.uint64(delta)
        assert check_blobs(case.batch, bad), (f, delta)
    bad = dict(rows); bad["seq"] = rows["seq"][:-16]
    assert check_blobs(case.batch, bad)
    empty = np.nonzero(lq == 0)[0]
    assert len(empty)                                                                # a record of no bases has no interval: any aligned offset inside will do
    ok = dict(rows); ok["seq_off"] = rows["seq_off"].copy(); ok["seq_off"][empty] = 0
    assert not check_blobs(case.batch, ok)
