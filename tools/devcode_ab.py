#!/usr/bin/env python3
"""Device code of two builds of libsegnb_hip.so, kernel by kernel (no GPU needed): for a change that must not touch a kernel.

    python tools/devcode_ab.py PARENT_CSRC CANDIDATE_CSRC > profiles/NAME.txt

Both directories were built with csrc/build.sh (obj/*.o and libsegnb_hip.so in place).  The gfx950 code object of every obj/*.o
is extracted with llvm-objdump --offloading and compared:

  (i)   the set of kernel symbols of the whole library (a kernel may move between objects);
  (ii)  per kernel, the disassembly -- mnemonics, operands and encoding words; the addresses in front of them and the s_nop
        padding behind the last instruction are dropped -- and
        the 64 bytes of its kernel descriptor, without kernel_code_entry_byte_offset (bytes 16..23: where the code lies
        relative to the descriptor, which changes when a kernel moves to another object);
  (iii) the segnb_* symbols the two shared libraries export.

Exit status 0 if nothing differs.
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()


def code_objects(csrc, tmp):
    """[(object name, path of its extracted gfx950 code object)]"""
    out = []
    for o in sorted(glob.glob(os.path.join(csrc, 'obj', '*.o'))):
        d = os.path.join(tmp, os.path.basename(o))
        os.makedirs(d)
        # (the bundles are written beside the path given: a link in the scratch directory keeps them out of obj/)
        os.symlink(os.path.abspath(o), os.path.join(d, os.path.basename(o)))
        run(os.path.join(LLVM, 'llvm-objdump'), '--offloading', os.path.basename(o), cwd=d)
        found = glob.glob(os.path.join(d, '*gfx950*'))
        assert len(found) <= 1, (o, found)
        if found:                       # (an object without kernels has no bundle)
            out.append((os.path.basename(o), found[0]))
    return out


def sections(path):
    """{section name: (address, file offset, size)}"""
    out = {}
    for line in run(os.path.join(LLVM, 'llvm-readelf'), '-S', '-W', path).splitlines():
        m = re.match(r'\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', line)
        if m:
            out[m.group(1)] = (int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16))
    return out


def kernels(path):
    """{kernel symbol: (normalised disassembly, descriptor bytes without the entry offset)}"""
    with open(path, 'rb') as f:
        blob = f.read()
    secs = sections(path)
    desc = {}
    for line in run(os.path.join(LLVM, 'llvm-readelf'), '-s', '-W', '--dyn-syms', path).splitlines():
        p = line.split()
        if len(p) == 8 and p[3] == 'OBJECT' and p[7].endswith('.kd'):
            addr, size = int(p[1], 16), int(p[2])
            assert size == 64, line
            for a, off, sz in secs.values():
                if a <= addr < a + sz and a != 0:
                    kd = blob[off + addr - a: off + addr - a + 64]
                    desc[p[7][:-3]] = kd[:16] + kd[24:]
    text, name = {}, None
    for line in run(os.path.join(LLVM, 'llvm-objdump'), '-d', path).splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            name = m.group(1)
            text[name] = []
        elif name is not None and '//' in line:
            ins, _, rest = line.partition('//')
            enc = rest.split(':', 1)[1].split('<')[0]
            text[name].append(ins.strip() + ' | ' + ' '.join(enc.split()))
    assert set(desc) <= set(text), sorted(set(desc) - set(text))[:5]
    for t in text.values():             # the s_nop padding up to the next kernel (or the end of the section) is no code
        while t and t[-1].startswith('s_nop 0 '):
            t.pop()
    return {k: ('\n'.join(text[k]), desc[k]) for k in desc}


def library(csrc, tmp):
    """{kernel: (object, text, descriptor)}"""
    out = {}
    for obj, path in code_objects(csrc, tmp):
        for k, (t, d) in kernels(path).items():
            assert k not in out or out[k][1:] == (t, d), ('one kernel, two bodies', k, obj, out[k][0])
            out.setdefault(k, (obj, t, d))
    return out


def exported(csrc):
    names = []
    for line in run(os.path.join(LLVM, 'llvm-readelf'), '-W', '--dyn-syms', os.path.join(csrc, 'libsegnb_hip.so')).splitlines():
        p = line.split()
        if len(p) == 8 and p[3] == 'FUNC' and p[6] != 'UND' and p[7].startswith('segnb_'):
            names.append(p[7])
    return sorted(names)


def main(parent, cand):
    bad = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a, b = library(parent, ta), library(cand, tb)
    print('kernels: parent %d, candidate %d' % (len(a), len(b)))
    for k in sorted(set(a) - set(b)):
        print('ONLY IN PARENT   ', k)
    for k in sorted(set(b) - set(a)):
        print('ONLY IN CANDIDATE', k)
    bad += len(set(a) ^ set(b))
    moved = same = 0
    for k in sorted(set(a) & set(b)):
        moved += a[k][0] != b[k][0]
        dt, dd = a[k][1] != b[k][1], a[k][2] != b[k][2]
        if dt or dd:
            bad += 1
            print('DIFFERS (%s%s) %s: %s -> %s' % ('text' if dt else '', ' descriptor' if dd else '', k, a[k][0], b[k][0]))
        else:
            same += 1
    print('identical disassembly and kernel descriptor: %d of %d kernels (%d of them in another object file)' % (same, len(set(a) & set(b)), moved))
    for k in sorted(set(a) & set(b)):
        if a[k][0] != b[k][0]:
            print('  moved %s -> %s: %s' % (a[k][0], b[k][0], k))
    ea, eb = exported(parent), exported(cand)
    print('exported segnb_* symbols: parent %d, candidate %d, %s' % (len(ea), len(eb), 'identical' if ea == eb else 'DIFFERENT'))
    for n in sorted(set(ea) ^ set(eb)):
        print('EXPORT DIFFERS', n)
    bad += ea != eb
    print('RESULT:', 'no difference' if not bad else '%d difference(s)' % bad)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
