"""CPU: the device JSONL decoder's host-compilable core (csrc/jsonl_dev.h: the
per-record parser, the per-history sequential pass and the section layout)
under the host sanitizers.

tests/jsonl_dev_host is a stand-alone program built with
-fsanitize=address,undefined (it alone; it links the uninstrumented
libs2lincheck.so, and nothing is loaded into this Python process). It drives
the core serially over the GPU tests' corpus (test_jsonl_device.py tests 1-3, 5
and 6) and compares with s2lc_load_jsonl: the accept / refuse decision,
per-event fields, K, n_tokens and the section bytes against
s2lc_history_save_many's. It exits 0 only when every history agrees and no
sanitizer reported."""
import os
import shutil
import subprocess

import pytest

import jsonl_dev_corpus as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "s2_verification_amd")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC) or shutil.which("make") is None:
        pytest.skip("no compiler")
    if not os.path.exists(os.path.join(LIBDIR, "libs2lincheck.so")):
        pytest.skip("libs2lincheck.so not built")
    out = str(tmp_path_factory.mktemp("jdh") / "jsonl_dev_host")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "jsonl_dev_host"), "OUT=" + out, "HIPCC=" + HIPCC],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return out


def test_core_matches_the_cpu_decoder_under_sanitizers(program, tmp_path):
    cases = []  # (expectation, blob): + the core must accept, - must refuse, ? whatever the CPU decoder allows
    cases += [("+", b) for b in C.golden_blobs()[1]]
    cases += [("+", b) for _, b in C.sim_blobs()]
    for v, where, b in C.integer_blobs():
        cases.append(("?", b))
    for form, b in C.fallback_variants():
        cases.append(("+" if form else "-", b))
    cases.append(("-", C.many_tokens_blob()))
    cases.append(("+", C.token_blob()))
    cases.append(("+", b""))
    args = []
    for i, (exp, b) in enumerate(cases):
        p = tmp_path / ("h%04d.jsonl" % i)
        p.write_bytes(b)
        args.append(exp + str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r =subprocess.run([program] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d histories, 0 failures" % (len(cases) + 12) in r.stdout
