"""The corpus of the device JSONL decoder's tests (test_jsonl_device.py on the
GPU, test_jsonl_dev_host.py through the host-compiled core): collector JSONL
blobs, and for the variants whether they are still in the collector's form."""
import functools
import os

import s2_verification_amd as s2
from s2_verification_amd import workloads as W
from helpers import GOLDEN


@functools.lru_cache(None)
def golden_blobs():
    names = sorted(f for f in os.listdir(GOLDEN) if f.startswith("ref_") and f.endswith(".jsonl"))
    assert len(names) == 8
    return names, [open(os.path.join(GOLDEN, f), "rb").read() for f in names]


@functools.lru_cache(None)
def c4_blobs(n=24):
    return [s2.simulate_jsonl(**W.c4_params(sd)) for sd in range(n)]


@functools.lru_cache(None)
def sim_blobs():
    """(name, blob): C4 seeds 0..23, C3 (16 tokens, 19 chains), test_loader's
    48 x 12 history (48 chains), A144 (> 128 chains)."""
    out = [("c4-%d" % sd, b) for sd, b in enumerate(c4_blobs())]
    out.append(("C3", W.config_jsonl("C3")))
    out.append(("48x12", s2.simulate_jsonl(workflow=0, num_clients=48, ops_per_client=12, seed=9, p_indefinite=0.05)))
    out.append(("A144", W.config_jsonl("A144")))
    return out


def integer_values():
    """test_loader.py::test_fast_path_integers_at_every_length's value list."""
    vals = ["0", "01", "00"]
    for k in range(1, 21):
        vals += [str(10 ** k - 1), str(10 ** (k - 1)), "1234567890123456789012"[:k]]
    vals += ["18446744073709551615", "18446744073709551616", "18446744073709551625", "18446744073709552615",
             "18440000000000000000", "18449999999999999999", "18450000000000000000", "99999999999999999999",
             "184467440737095516150", "9223372036854775807", "9223372036854775808"]
    return vals


def integer_blobs():
    """(value, position, blob) with the value in each of the four positions."""
    out = []
    for v in integer_values():
        for where in ("hash", "tail", "client", "op"):
            h = v if where == "hash" else "5"
            t = v if where == "tail" else "3"
            c = v if where == "client" else "1"
            o = v if where == "op" else "0"
            data = ('{"event":{"Start":{"Append":{"num_records":1,"record_hashes":[%s],"set_fencing_token":null,'
                    '"fencing_token":null,"match_seq_num":%s}}},"client_id":%s,"op_id":%s}\n'
                    '{"event":{"Finish":{"ReadSuccess":{"tail":%s,"stream_hash":%s}}},"client_id":%s,"op_id":%s}\n'
                    % (h, t, c, o, t, h, c, o)).encode()
            out.append((v, where, data))
    return out


def boundary_blobs(n=288):
    """Small histories whose record lengths step by one byte (the client_id's
    digit count, the token's length), with and without the final newline:
    concatenated in one chunk, record starts land on every offset modulo the
    kernels' 16-byte and 4096-byte tiles. (two_records, blob): a one-op history
    (Start + Finish), or its Start alone (an op never returned)."""
    out = []
    for i in range(n):
        cid = "1" * (1 + i % 19)
        tok = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJ"[:i % 33]
        start = ('{"event":{"Start":{"Append":{"num_records":1,"record_hashes":[%d],"set_fencing_token":"%s",'
                 '"fencing_token":null,"match_seq_num":null}}},"client_id":%s,"op_id":0}' % (i, tok, cid))
        fin = '{"event":{"Finish":{"AppendSuccess":{"tail":1}}},"client_id":%s,"op_id":0}' % cid
        two = i % 5 != 4
        text = start + "\n" + fin if two else start
        if i % 2:
            text += "\n"
        out.append((two, text.encode()))
    return out


# (old, new, still in the collector's form)
_PERTURB = (('":', '": ', False), ('"event"', '"Event"', False), ('"client_id":', '"client_id":-', False),
            ('"op_id":', '"op_id":0', False), ('"tail":', '"tail":1.5e', False),
            ('"num_records":', '"num_records":1', False),
            ('"set_fencing_token":null', '"set_fencing_token":"t\\u00e9"', False),
            ('"fencing_token":null', '"fencing_token":"éx"', False), (',"op_id"', ',"x":[1,2],"op_id"', False),
            ('}\n', '}  ', False), ('{"event"', '\t{"event"', False), ('"Read"', '"Re\\u0061d"', False),
            # a match_seq_num is a field the collector writes: the record keeps its form
            ('"match_seq_num":null', '"match_seq_num":7', True), ('[', '[ ', False))


def perturbations(text):
    """test_loader.py::_perturbations re-stated: variants of a collector-format
    blob that leave the collector's form or are invalid, each with whether it
    is still in that form. (collector_form, text)."""
    lines = text.splitlines(keepends=True)
    out = []
    for i in range(0, min(len(lines), 40), 7):
        ln = lines[i]
        for a, b, form in _PERTURB:
            if a in ln:
                out.append((form, "".join(lines[:i] + [ln.replace(a, b, 1)] + lines[i + 1:])))
    return out


def structural_variants(text):
    """test_loader.py::_structural_variants re-stated: op ids not 0, 1, 2, ...
    in call order, a second Finish, an op never returned, a Finish before its
    Start. None is a history the device decodes. (collector_form, text)."""
    lines = text.splitlines(keepends=True)
    out = [text.replace('"op_id":', '"op_id":1', 1)]
    fin = [i for i, ln in enumerate(lines) if '"Finish"' in ln]
    if fin:
        out.append("".join(lines + [lines[fin[len(fin) // 2]]]))
        out.append("".join(lines[:fin[-1]] + lines[fin[-1] + 1:]))
        i = fin[0]
        out.append("".join([lines[i]] + lines[:i] + lines[i + 1:]))
    return [(False, v) for v in out]


@functools.lru_cache(None)
def fallback_variants():
    """(collector_form, blob) over 4 blobs: two C4 histories, C4's first
    fencing history and a golden file."""
    c4 = c4_blobs()
    base = [c4[0], c4[1], c4[2], golden_blobs()[1][0]]
    out = []
    for b in base:
        out += perturbations(b.decode())
        out += structural_variants(b.decode())
    return [(form, v.encode("utf-8")) for form, v in out]


def many_tokens_blob(n=6000):
    """test_loader.py::test_many_distinct_fencing_tokens' history: n distinct tokens."""
    lines = []
    for i in range(n):
        lines.append('{"event":{"Start":{"Append":{"num_records":0,"record_hashes":[],"set_fencing_token":"s%d",'
                     '"fencing_token":%s,"match_seq_num":null}}},"client_id":1,"op_id":%d}'
                     % (i, '"s%d"' % (i // 2) if i % 3 else "null", i))
        lines.append('{"event":{"Finish":"AppendDefiniteFailure"},"client_id":1,"op_id":%d}' % i)
    return "\n".join(lines).encode()


def token_blob():
    """Exactly 64 distinct tokens (the device cap), of 0 to 64 bytes; set and
    batch tokens differ within a record, a batch token can be new (interned
    after the record's set token), and tokens are reused."""
    toks = [("%02d" % i + "x" * 64)[:i + 1] for i in range(63)] + [""]
    assert len(set(toks)) == 64 and max(map(len, toks)) == 63
    toks[62] = "y" * 64
    lines = []
    for i in range(96):
        if i < 32:
            st, bt = toks[2 * i], toks[2 * i + 1]  # both new: set first, then batch
        else:
            st, bt = toks[(7 * i) % 64], (toks[(3 * i) % 64] if i % 4 else None)
        lines.append('{"event":{"Start":{"Append":{"num_records":0,"record_hashes":[],"set_fencing_token":"%s",'
                     '"fencing_token":%s,"match_seq_num":null}}},"client_id":1,"op_id":%d}'
                     % (st, "null" if bt is None else '"%s"' % bt, i))
        lines.append('{"event":{"Finish":"AppendDefiniteFailure"},"client_id":1,"op_id":%d}' % i)
    return ("\n".join(lines) + "\n").encode()
