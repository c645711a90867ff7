"""csrc/sha256.h -- the statement writer of a bound membership proof ("ZKMB") and the length / block-count functions of its challenge hash -- as a stand-alone
host program: tests/host_arith/host_member_bound.cpp, built with plain g++.  For n = 1, 2, 3, 4, 8, 9, 12 it hashes 4 n made-up points || S_b the two ways the
engine does (byte stream; padded blocks) and prints inputs and digests; here the message is rebuilt from the inputs with tests/member_bound_common.py's
statement_bytes and hashed with hashlib.  The unpadded length is 268 n + 152: 36, 48, 60, 8, 56, 4, 40 bytes into the last block -- n = 3 and n = 8 spill
their padding into an extra block, n = 4 and n = 9 sit just behind a boundary.  Once more under the address and undefined-behaviour sanitizers."""
import hashlib
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_member_bound.cpp')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import member_bound_common as MB   # noqa: E402

NS = [1, 2, 3, 4, 8, 9, 12]
TAIL = [36, 48, 60, 8, 56, 4, 40]


def _run(tmp_path, name, *flags):
    assert shutil.which('g++') is not None, 'g++ is needed to build tests/host_arith/host_member_bound.cpp'
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', *flags, '-I' + CSRC, SRC, '-o', exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'member bound hash ok' and len(lines) == len(NS) + 1
    return [dict(f.split('=') for f in ln.split()) for ln in lines[:-1]]


def _check(recs):
    for n, tail, r in zip(NS, TAIL, recs):
        assert int(r['n']) == n and int(r['len']) == 268 * n + 152 and int(r['len']) % 64 == tail
        coords = bytes.fromhex(r['coords'])
        assert len(coords) == 8 * n * 33
        points = b''.join(b'\x04' + coords[66 * k:66 * k + 66] for k in range(4 * n))
        s_b = MB.statement_bytes(bytes.fromhex(r['digest']), bytes.fromhex(r['context']), b'\x04' + bytes.fromhex(r['com']))
        msg = points + s_b
        assert len(msg) == int(r['len']) and len(s_b) == MB.STATEMENT_BYTES == 152
        assert int(r['blocks']) == (len(msg) + 9 + 63) // 64
        want = hashlib.sha256(msg).hexdigest()
        assert r['stream'] == want, n
        assert r['blockwise'] == want, n
    spills = [int(r['n']) for r in recs if int(r['blocks']) == int(r['len']) // 64 + 2]
    assert spills == [3, 8]   # the sizes whose 0x80 and length do not fit behind the message's last bytes


def test_statement_hash_agrees_with_hashlib(tmp_path):
    _check(_run(tmp_path, 'host_member_bound', '-O1'))


def test_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _check(_run(tmp_path, 'host_member_bound_san', '-O0', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'))
