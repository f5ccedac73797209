"""GPU: collector JSONL decoded on the device into binary cache sections
(csrc/jsonl_dev.hip, s2lc_load_jsonl_many_device / Checker.load_jsonl_many).

Every test compares the device call with s2.load_many on the same blobs by
info(), events() and save_cache([h]) bytes; on_device says which histories
the device decoded (the others took the host decoder inside the call), and
n_rejected (a device section the cache loader's checks refuse) must be 0."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import s2_verification_amd as s2
import jsonl_dev_corpus as C
from helpers import golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def canon(h):
    return (h.info(), h.events(), s2.save_cache([h]))


def cpu_one(blob):
    """load_many's result for one blob: ("ok", canon) or ("error", status, message after "history 0: ")."""
    try:
        h = s2.load_many([blob], threads=1)[0]
    except s2.S2LCError as e:
        msg = str(e)
        assert "history 0: " in msg
        return ("error", e.status, msg.split("history 0: ", 1)[1])
    return ("ok", canon(h))


def device_equals_cpu(checker, blobs, want_on_device=None):
    """One device call over blobs (all valid); each history equal to load_many's."""
    hs, st = checker.load_jsonl_many(blobs)
    ref = s2.load_many(blobs)
    assert len(hs) == len(ref) == len(blobs)
    for i, (a, b) in enumerate(zip(hs, ref)):
        assert canon(a) == canon(b), i
    assert st["n_rejected"] == 0
    on = st["on_device"].tolist()
    assert st["n_device"] == sum(on) and st["n_fallback"] == len(blobs) - sum(on)
    if want_on_device is not None:
        assert on == [int(x) for x in want_on_device], [i for i, (x, y) in enumerate(zip(on, want_on_device)) if x != y]
    return hs, st


def test_golden_files(checker):
    """1: all eight reference JSONL files decode on the device, the 105 KB single record included."""
    names, blobs = C.golden_blobs()
    assert max(len(b) for b in blobs) > 100000
    device_equals_cpu(checker, blobs, [1] * 8)


def test_simulated_histories(checker):
    """2: C4 seeds 0..23 (three workflows, tokens, injected violations), C3, 48 chains, > 128 chains."""
    sims = C.sim_blobs()
    blobs = [b for _, b in sims]
    hs, st = device_equals_cpu(checker, blobs, [1] * len(blobs))
    info = {name: h.info() for (name, _), h in zip(sims, hs)}
    assert info["C3"]["n_tokens"] == 16 and info["C3"]["n_chains"] == 19
    assert info["48x12"]["n_chains"] == 48 and info["A144"]["n_chains"] > 128
    res = checker.check_many(hs[:24])
    rows = golden("c4_verdicts.json")["rows"]
    assert [r.verdict for r in res] == [s2.Ok if rows[i][0] == "O" else s2.Illegal for i in range(24)]


def test_integers(checker):
    """3: test_fast_path_integers_at_every_length's values in each of the four
    positions. The valid ones are one batch, equal to the CPU's; every one is
    decoded on the device except an op id other than 0, which is in the
    collector's form as a record but not as a history (op ids count from 0:
    load_direct hands it to finalize too). An invalid one raises the CPU's
    error under its index."""
    cases = C.integer_blobs()
    cpu = [cpu_one(b) for _, _, b in cases]
    valid = [i for i, c in enumerate(cpu) if c[0] == "ok"]
    assert 0 < len(valid) < len(cases)
    want = [not (cases[i][1] == "op" and cases[i][0] != "0") for i in valid]
    hs, _ = device_equals_cpu(checker, [cases[i][2] for i in valid], want)
    for i, h in zip(valid, hs):
        assert canon(h) == cpu[i][1], cases[i][:2]
    good = cases[valid[0]][2]
    for i, c in enumerate(cpu):
        if c[0] == "ok":
            continue
        with pytest.raises(s2.S2LCError) as e:
            checker.load_jsonl_many([good, cases[i][2], good])
        assert e.value.status == c[1] and str(e.value).endswith("history 1: " + c[2]), cases[i][:2]


def test_boundary_sweep(checker):
    """4: >= 256 small histories whose record lengths step by one byte, one or
    two records each, with and without the final newline; a 0-byte buffer and
    a one-op history in the same batch; n = 0 on its own."""
    cases = C.boundary_blobs()
    assert len(cases) >= 256
    blobs = [b for _, b in cases]
    want = [two for two, _ in cases]
    lens = {len(b) % 16 for b in blobs}
    assert len(lens) == 16
    blobs.insert(100, b"")
    want.insert(100, True)  # no records: an empty history, decoded on the device
    assert not blobs[-1].endswith(b"\n") or not blobs[-2].endswith(b"\n")
    # end on a history without its final newline: its last record ends at the staged text's last byte
    if blobs[-1].endswith(b"\n"):
        blobs[-1], blobs[-2] = blobs[-2], blobs[-1]
        want[-1], want[-2] = want[-2], want[-1]
    device_equals_cpu(checker, blobs, want)
    hs, st = checker.load_jsonl_many([])
    assert hs == [] and st["n_device"] == 0 and st["n_fallback"] == 0 and len(st["on_device"]) == 0


def test_fallbacks(checker):
    """5: variants that leave the collector's form, mixed into one batch with
    accepted histories: those valid on the CPU are equal and decoded on the
    host (the one variant that keeps the collector's form, a match_seq_num
    value, on the device), the untouched histories stay on the device. An
    invalid one raises the CPU's error under the lowest index."""
    variants = C.fallback_variants()
    cpu = [cpu_one(b) for _, b in variants]
    valid = [i for i, c in enumerate(cpu) if c[0] == "ok"]
    invalid = [i for i, c in enumerate(cpu) if c[0] == "error"]
    assert len(valid) >= 20 and len(invalid) >= 8
    assert sum(1 for i in valid if variants[i][0]) >= 1
    c4 = C.c4_blobs()
    blobs, want = [], []
    for k, i in enumerate(valid):
        blobs.append(variants[i][1])
        want.append(variants[i][0])
        if k % 3 == 0:
            blobs.append(c4[4 + k % 20])
            want.append(True)
    device_equals_cpu(checker, blobs, want)
    batch = [c4[k] for k in range(6)]
    batch[4] = variants[invalid[0]][1]
    batch[2] = variants[invalid[-1]][1]
    with pytest.raises(s2.S2LCError) as e:
        checker.load_jsonl_many(batch)
    c = cpu[invalid[-1]]
    assert e.value.status == c[1] and str(e.value).endswith("history 2: " + c[2])
    big = C.many_tokens_blob()
    device_equals_cpu(checker, [c4[0], big, c4[1]], [1, 0, 1])


def test_tokens(checker):
    """6: 64 distinct tokens (the cap) of 0..64 bytes, set != batch token, a new
    batch token interned after its record's set token, reused tokens."""
    hs, _ = device_equals_cpu(checker, [C.token_blob(), C.c4_blobs()[2]], [1, 1])
    assert hs[0].info()["n_tokens"] == 64


_CHILD = r"""
import hashlib, json, sys
sys.path[:0] = [%r, %r]
import s2_verification_amd as s2
import jsonl_dev_corpus as C
blobs = list(C.c4_blobs()) + [s2.simulate_jsonl(workflow=0, num_clients=8, ops_per_client=1500, seed=4)]
hs, st = s2.Checker().load_jsonl_many(blobs)
print(json.dumps({"sha": hashlib.sha256(s2.save_cache(hs)).hexdigest(), "on": st["on_device"].tolist(),
                  "bytes_in": st["bytes_in"], "max": max(map(len, blobs)), "rejected": st["n_rejected"]}))
"""


def test_chunking(checker):
    """7: S2LC_DEVDECODE_CHUNK_MB=1 in a fresh child process: 24 C4 histories
    take >= 4 chunks and one history is larger than the chunk; the result
    equals this process's one-chunk result."""
    blobs = list(C.c4_blobs()) + [s2.simulate_jsonl(workflow=0, num_clients=8, ops_per_client=1500, seed=4)]
    assert sum(map(len, blobs[:24])) >= 3 << 20 and len(blobs[24]) > 1 << 20
    hs, st = device_equals_cpu(checker, blobs, [1] * 25)
    env = dict(os.environ, S2LC_DEVDECODE_CHUNK_MB="1")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["max"] == len(blobs[24]) and out["rejected"] == 0
    assert out["on"] == [1] * 25
    assert out["sha"] == hashlib.sha256(s2.save_cache(hs)).hexdigest()


def test_pipeline(checker):
    """8: check_jsonl_many(decode="device") returns decode="host"'s arrays exactly."""
    blobs = C.c4_blobs(64)
    host = checker.check_jsonl_many(blobs, slices=2, decode="host")
    dev = checker.check_jsonl_many(blobs, slices=2, decode="device")
    assert set(host) == set(dev)
    for k in host:
        assert host[k].dtype == dev[k].dtype and np.array_equal(host[k], dev[k]), k
    assert int((host["verdict"] == s2.S2LC_OK).sum()) > 0
