"""Per-kernel ISA comparison of two builds of libpcgan_hip.so (CPU only):  python scripts/isa_diff.py A.so B.so

For every function symbol of the gfx950 code objects of both libraries it compares
  (a) the instruction text, addresses, encodings and the alignment padding behind the last instruction stripped, and
  (b) the values of the kernel's metadata that decide occupancy: VGPR, AGPR and SGPR count, LDS bytes, scratch bytes,
and prints the symbols only in A, only in B, and those that differ.  Exit status 1 if any of the three lists is non-empty.
A refactor that moves kernels between translation units is checked with this: identical instructions under identical budgets.

code_objects() and instructions() are also what tests/test_isa_guard.py walks the library with."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM_BIN = '/opt/rocm/lib/llvm/bin'
OBJDUMP = os.path.join(LLVM_BIN, 'llvm-objdump')
READELF = os.path.join(LLVM_BIN, 'llvm-readelf')
PADDING = ('...', 's_code_end')      # llvm-objdump's elision of zero bytes; the filler behind the last function of a code object
BUDGET_KEYS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')


def code_objects(lib, tmp):
    """unbundle a copy of `lib` inside the directory `tmp`; returns the paths of its gfx950 code objects"""
    work = os.path.join(tmp, 'lib.so')
    shutil.copy(lib, work)
    subprocess.run([OBJDUMP, '--offloading', work], cwd=tmp, check=True, capture_output=True)
    return sorted(glob.glob(work + '.*gfx950*'))


def instructions(obj):
    """disassemble one code object: yields (symbol, line) for every line below a `<symbol>:` header (symbol None above the first)"""
    cur = None
    p = subprocess.Popen([OBJDUMP, '-d', obj], stdout=subprocess.PIPE, text=True)
    for line in p.stdout:
        m = re.match(r'^[0-9a-f]+ <(.+)>:', line)
        if m:
            cur = m.group(1)
            continue
        yield cur, line
    p.wait()


def budgets(obj):
    """{kernel name: {key: value}} from the code object's AMDGPU metadata note, BUDGET_KEYS only"""
    out, cur = {}, None
    text = subprocess.run([READELF, '--notes', obj], check=True, capture_output=True, text=True).stdout
    for line in text.splitlines():
        m = re.match(r'^  (- | {2})(\.\w+):\s*(.*)$', line)      # a key of a kernel's own map ('- ' opens the next kernel)
        if not m:
            continue
        if m.group(1) == '- ':
            cur = {}
        if cur is None:
            continue
        if m.group(2) == '.name':
            out[m.group(3)] = cur
        elif m.group(2) in BUDGET_KEYS:
            cur[m.group(2)] = m.group(3)
    return out


def describe(lib):
    """{symbol: (tuple of instruction texts, budgets or None)} over all gfx950 code objects of `lib`"""
    tmp = tempfile.mkdtemp(prefix='pcgan_isa_')
    try:
        objs = code_objects(lib, tmp)
        if not objs:
            raise SystemExit('%s: no gfx950 code object' % lib)
        code, meta = {}, {}
        for o in objs:
            for sym, line in instructions(o):
                text = line.split('//')[0].strip()
                if sym is not None and text:
                    code.setdefault(sym, []).append(text)
            meta.update(budgets(o))
        for c in code.values():          # what follows the last instruction pads the function to the next one's alignment
            while c and (c[-1] in PADDING or c[-1].startswith('s_nop')):
                c.pop()
        return {s: (tuple(c), meta.get(s)) for s, c in code.items()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__.split('\n')[0])
    a, b = describe(argv[1]), describe(argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = []
    for s in sorted(set(a) & set(b)):
        (ca, ma), (cb, mb) = a[s], b[s]
        if ca != cb or ma != mb:
            what = []
            if ca != cb:
                what.append('instructions %d -> %d' % (len(ca), len(cb)))
            what += ['%s %s -> %s' % (k, ma.get(k), mb.get(k)) for k in BUDGET_KEYS if ma and mb and ma.get(k) != mb.get(k)]
            differ.append('%s: %s' % (s, ', '.join(what) or 'metadata present in one only'))
    kernels = sum(1 for v in b.values() if v[1] is not None)
    print('%d symbols in A, %d in B (%d kernels with metadata in B)' % (len(a), len(b), kernels))
    for title, items in (('only in A', only_a), ('only in B', only_b), ('different', differ)):
        print('%s: %d' % (title, len(items)))
        for i in items:
            print('  ' + i)
    return 1 if (only_a or only_b or differ) else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
