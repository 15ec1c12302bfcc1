"""The parity generator itself (tests/fuzzgen.py, CPU only): options added to make_case must leave the cases of the existing seeds byte for
byte as they were, since every GPU parity test and fuzz sweep names its cases by seed."""
import hashlib
import json

import numpy as np
import pytest

import fuzzgen
from gencore_amd.batch import ReadBatch


def case_digest(batch, over, reference, contig_len):
    h = hashlib.sha256()
    for f in ReadBatch.FIELDS:
        a = getattr(batch, f)
        h.update(f.encode()); h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    h.update(json.dumps(over, sort_keys=True).encode())
    for nib, ln in reference:
        h.update(str(ln).encode()); h.update(b"-" if nib is None else nib.tobytes())
    h.update(json.dumps(list(contig_len)).encode())
    return h.hexdigest()[:16]


# frozen from the generator as it was before thresholds= / scores= / deep_mols= existed
FROZEN = [(0, {}, "70d9fe98130bd3e8"), (5, {}, "0640102d7a44d6aa"), (17, {}, "c30b591d00fdfde0"), (31, dict(n_mol=50), "3755c737f68dd3ad"),
          (103, dict(umi_mode="colon", period=3), "0aa8b92691f8c4cc"), (200, dict(n_mol=6, umi_mode="none", deep=70), "bee46274085fbaa6"),
          (605, dict(n_mol=50, exotic=True), "6ccbc618c33f5bd4")]


@pytest.mark.parametrize("seed,kw,digest", FROZEN)
def test_existing_seeds_generate_the_same_cases(oracle, seed, kw, digest):
    assert case_digest(*fuzzgen.make_case(seed, **kw)) == digest


def test_threshold_and_score_options(oracle):
    assert fuzzgen.quals_around((25, 25, 25)) == [0, 2, 24, 25, 26, 40]
    assert fuzzgen.quals_around((20, 15, 8)) == [0, 2, 7, 8, 9, 14, 15, 16, 19, 20, 21, 40]
    batch, over, reference, contig_len = fuzzgen.make_case(3, thresholds=(40, 35, 30), scores=(10, 7, 3, 1))
    assert (over["high_quality"], over["moderate_quality"], over["low_quality"]) == (40, 35, 30)
    assert (over["score_high"], over["score_moderate"], over["score_low"], over["score_bad"]) == (10, 7, 3, 1)
    assert set(np.unique(batch.qual).tolist()) <= set(fuzzgen.quals_around((40, 35, 30))) | {20, 37}      # (37: the mostly-good reads; 20: unmapped reads)
    p = fuzzgen.make_params(over, contig_len)
    assert (p.high_quality, p.moderate_quality, p.low_quality, p.score_bad) == (40, 35, 30, 1)
    # deep_mols: the first k molecules at depth `deep`
    b1 = fuzzgen.make_case(4, n_mol=6, umi_mode="none", deep=90)[0]
    b3 = fuzzgen.make_case(4, n_mol=6, umi_mode="none", deep=90, deep_mols=3)[0]
    assert b3.n > b1.n + 300
