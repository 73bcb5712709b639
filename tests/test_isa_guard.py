"""CPU: guards on the ISA of the built library (llvm-objdump of libpcgan_hip.so's gfx950 code objects).

Round 3 found one kernel whose sums differed from run to run beside f16-MFMA kernels of another stream; round 4's ISA study
(scripts/micro/head_wgrad_isa.md) excluded a compiler wait-count bug and isolated the one instruction form unique to the failing
build: packed fp32 arithmetic with `op_sel:[0,1,0]` (high dword of src1 broadcast to both lanes).  The cause is not established, so the
form is banned from the library: this test fails if any kernel contains it."""
import os
import re
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'pc-gan_amd', 'lib', 'libpcgan_hip.so')
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from isa_diff import OBJDUMP, code_objects, instructions      # noqa: E402  (the extract-and-disassemble walk, shared with the script)


@pytest.mark.timeout(600)
def test_no_packed_fp32_high_broadcast_form_in_the_library():
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip('library or llvm-objdump not present (build() first)')
    tmp = tempfile.mkdtemp(prefix='pcgan_isa_')
    try:
        objs = code_objects(LIB, tmp)
        assert objs, 'no gfx950 code object in the library'
        bad, packed, kernels = [], 0, set()
        for o in objs:
            for cur, line in instructions(o):
                if 'v_pk_' in line and '_f32' in line:
                    packed += 1
                    kernels.add(cur)
                    code = line.split('//')[0]
                    if re.search(r'op_sel:\[0,1,0\]', code) and 'op_sel_hi' not in code:
                        bad.append((cur, code.strip()))
        assert packed > 0, 'disassembly found no packed fp32 instruction at all: the scan is broken'
        assert not bad, 'packed fp32 op_sel:[0,1,0] form (scripts/micro/head_wgrad_isa.md) in: %s' % sorted({b[0] for b in bad})[:5]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.mark.timeout(600)
def test_row_ring_kernels_keep_scalar_loads_out_of_their_stage_loops():
    """csrc/wgrad_rowring.hip ends a stage with `s_waitcnt lgkmcnt(N)` + a raw `s_barrier`: "the row's LDS writes are older than the N
    newest LDS operations, so they have completed".  That holds because a wave's LDS operations return in order -- scalar memory loads count
    on the same counter and return OUT of order, so none may be in flight there.  Guard: in both kernels every s_load / s_buffer_load sits in
    front of the first matrix instruction (kernel arguments, read once), and the counted waits are the ones the source asks for."""
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip('library or llvm-objdump not present (build() first)')
    tmp = tempfile.mkdtemp(prefix='pcgan_isa_')
    try:
        seen = {}
        for o in code_objects(LIB, tmp):
            for cur, line in instructions(o):
                if cur is None or 'rowring_wgrad' not in cur:
                    continue
                seen.setdefault(cur, {'mfma': False, 'late_sload': [], 'waits': set()})
                code = line.split('//')[0]
                if 'v_mfma' in code:
                    seen[cur]['mfma'] = True
                elif re.search(r'\bs_(buffer_)?load_', code) and seen[cur]['mfma']:
                    seen[cur]['late_sload'].append(code.strip())
                w = re.search(r's_waitcnt lgkmcnt\((\d+)\)\s*$', code.strip())
                if w:
                    seen[cur]['waits'].add(int(w.group(1)))
        assert len(seen) == 2, 'expected the fp32 and the bf16 row-ring kernel, found %r' % sorted(seen)
        for k, v in seen.items():
            assert v['mfma'] and not v['late_sload'], '%s: scalar loads behind the first MFMA: %r' % (k, v['late_sload'][:3])
            assert (4 if 'bf16' in k else 8) in v['waits'], '%s: the counted end-of-stage wait is gone (%r)' % (k, sorted(v['waits']))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
