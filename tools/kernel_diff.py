#!/usr/bin/env python3
"""Compare the gfx950 kernels of two sets of `hipcc --cuda-device-only -S` files.

    kernel_diff.py --old a.s [b.s ...] --new c.s [d.s ...]

Kernels are paired by demangled name with `(anonymous namespace)::` dropped, so a kernel may move
to another translation unit and its argument types to another namespace. Per kernel the table says
whether the instruction text and the descriptor (the .amdhsa_kernel block and the kernel's
metadata entry: registers, LDS, scratch, workgroup size, arguments) are identical once comments,
trailing blanks and local label numbers are stripped. The compiler numbers its private constants
(.str, .str.N) per file, so a reference to one is compared by what the constant holds, not by its
number: the same instructions over constants of different content are DIFFERENT. Exit status 1 on any difference, on a
kernel that only one side has, and on a kernel that a side has more than once.
"""
import re
import shutil
import subprocess
import sys

# a compiler-generated private constant (.str, .str.N): a reference, and its definition's label
PRIVATE = re.compile(r'(?<![\w.])\.str(\.\d+)?(?![\w.])')
PRIVATE_DEF = re.compile(r'\.str(\.\d+)?:$')

def kernels(path, out):
    """out[name] = list of (instruction text, descriptor) of the kernels in one assembly file"""
    filt = shutil.which('c++filt') or '/opt/rocm/llvm/bin/llvm-cxxfilt'
    text = subprocess.run([filt], input=open(path).read(), stdout=subprocess.PIPE, text=True,
                          check=True).stdout.replace('(anonymous namespace)::', '')
    lines = [re.sub(r'\.L([A-Za-z]+)\d+', r'.L\1', ln.split(';')[0].rstrip()) for ln in text.split('\n')]
    # consts[symbol] = the data directives of a private constant, as written (label .. .size)
    consts, raw = {}, text.split('\n')
    for i, ln in enumerate(raw):
        if PRIVATE_DEF.match(ln):
            j = next(k for k in range(i + 1, len(raw)) if raw[k].startswith('\t.size'))
            consts[ln[:-1]] = '\n'.join(raw[i + 1:j])
    meta = {}
    body = '\n'.join(lines)
    k0, k1 = body.find('amdhsa.kernels:'), body.find('amdhsa.target:')
    for entry in re.split(r'\n  - (?=\.)', body[k0:k1])[1:]:
        meta[re.search(r'^    \.name:\s+(.*)$', entry, re.M).group(1).strip("'")] = entry
    for d0, ln in enumerate(lines):
        if not ln.strip().startswith('.amdhsa_kernel '):
            continue
        name = ln.strip()[len('.amdhsa_kernel '):]
        start = lines.index(name + ':')
        end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
        d1 = lines.index('\t.end_amdhsa_kernel', d0)
        assert start < d0 < d1 < end, name
        # (the section switches around the descriptor carry the mangled name)
        code = [x for x in lines[start + 1:d0] + lines[d1 + 1:end]
                if x.strip() and not x.startswith(('\t.section', '\t.text'))]
        # the compiler numbers its private constants per file: compare what each reference holds
        refs = [m.group(0) for x in code for m in PRIVATE.finditer(x)]
        code = [PRIVATE.sub('.str', x) for x in code] + ['.str = ' + consts.get(r, 'undefined') for r in refs]
        desc = [x for x in lines[d0 + 1:d1] if x.strip()] + [meta[name].rstrip()]
        out.setdefault(name, []).append(('\n'.join(code), '\n'.join(desc)))


def main(argv):
    if '--old' not in argv or '--new' not in argv or argv.index('--old') > argv.index('--new'):
        sys.exit(__doc__)
    i, j = argv.index('--old'), argv.index('--new')
    old, new = {}, {}
    for p in argv[i + 1:j]:
        kernels(p, old)
    for p in argv[j + 1:]:
        kernels(p, new)
    bad = 0
    for name in sorted(set(old) | set(new)):
        a, b = old.get(name, []), new.get(name, [])
        if len(a) != 1 or len(b) != 1:
            verdict = 'UNPAIRED  old x%d  new x%d' % (len(a), len(b))
        else:
            verdict = 'text %s  descriptor %s' % tuple('same' if x == y else 'DIFFERENT'
                                                       for x, y in zip(a[0], b[0]))
        bad += 'same  descriptor same' not in verdict
        print('%-44s %s' % (verdict, name))
    print('%d kernels old, %d new, %d not identical' % (sum(map(len, old.values())),
                                                       sum(map(len, new.values())), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
