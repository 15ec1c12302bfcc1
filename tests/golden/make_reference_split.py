#!/usr/bin/env python
"""Freezes the answers of the reference's own tokenizer (src/util.h `split`, the test behind Cluster::isDuplex, cluster.cpp:246-258)
into reference_split.json, so that tests/test_oracle_known_answers.py needs no reference tree to check the oracle against them.
The answers come from oracle/_ref/libref_util.so (oracle/ref_probe: util.h compiled where it lies), which build() makes only
when the reference sources are present.  Run from the repo root after build():  python tests/golden/make_reference_split.py"""
import ctypes as C
import itertools
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PROBE = os.path.join(ROOT, "oracle", "_ref", "libref_util.so")

SPLIT = [("_A__B_", "_"), ("A_C", "_"), ("", "_"), ("_", "_"), ("__", "_"), ("A__C", "_"), ("ACGT_TTGA", "_")]


def duplex_cases():
    """Every UMI shape pair over a small alphabet (leading / trailing / doubled underscores, empty strings) + 3000 seeded random pairs."""
    alphabet = ["", "A", "AC", "_", "__", "A_", "_A", "A_C", "AC_GT", "GT_AC", "A__C", "_A_C", "A_C_", "A_C_G", "ACGT_TTGA", "TTGA_ACGT"]
    cases = list(itertools.product(alphabet, alphabet))
    rng = random.Random(7)
    for _ in range(3000):
        mk = lambda: "".join(rng.choice("ACGT_") for _ in range(rng.randint(0, 9)))
        a = mk()
        b = mk() if rng.random() < 0.5 else "_".join(reversed(a.split("_")))
        cases.append((a, b))
    return cases


def load_probe(path=PROBE):
    ref = C.CDLL(path)
    ref.ref_is_duplex.argtypes = [C.c_char_p, C.c_char_p]
    ref.ref_split.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    return ref


def probe_split(ref, s, sep):
    buf = C.create_string_buffer(256)
    n = ref.ref_split(s.encode(), sep.encode(), buf, 256)
    return n, buf.value.decode()


if __name__ == "__main__":
    ref = load_probe()
    split = [[s, sep] + list(probe_split(ref, s, sep)) for s, sep in SPLIT]
    duplex = [[a, b, int(bool(ref.ref_is_duplex(a.encode(), b.encode())))] for a, b in duplex_cases()]
    body = ",\n".join(json.dumps(x) for x in duplex)
    with open(os.path.join(HERE, "reference_split.json"), "w") as f:
        f.write('{\n "note": "answers of the reference tokenizer src/util.h split (oracle/ref_probe) and of the isDuplex decision built on it '
                '(cluster.cpp:246-258); [str, sep, token count, tokens joined by newline] / [umi1, umi2, is_duplex]",\n')
        f.write(' "split": %s,\n "is_duplex": [\n%s\n]\n}\n' % (json.dumps(split), body))
    print("%d split, %d is_duplex answers" % (len(split), len(duplex)))
