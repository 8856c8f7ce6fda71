#!/usr/bin/env python
"""Are the kernels of two sets of `hipcc -S --cuda-device-only` listings the same code?  (development aid: proof for a source move)

    python tools/isa_diff.py old1.s [old2.s ...] -- new1.s [new2.s ...]

Every kernel (`.amdhsa_kernel`) is keyed by its mangled name and compared from its entry label to `.end_amdhsa_kernel`: the whole body
and the whole descriptor.  Ignored: comments, blank lines, the number in `.LBB<n>_` / `.Lfunc_end<n>` (the kernel's index in its
listing), the kernel's own symbol where a line repeats it, and whether ConvArgs is named inside the anonymous namespace (`NS_8ConvArgsE`)
or at global scope (`8ConvArgs`).  Prints `same` / `DIFF` per kernel and the kernels found on one side only; exit status 1 on either."""
import re
import sys


def kernels(paths):
    found = {}
    for path in paths:
        text = open(path).read().replace('NS_8ConvArgsE', '8ConvArgs')
        for name in re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M):
            body = re.search(r'^%s:.*?^\s*\.end_amdhsa_kernel' % re.escape(name), text, re.S | re.M).group(0)
            lines = []
            for line in body.replace(name, '<kernel>').split('\n'):
                line = re.sub(r'\.(LBB|Lfunc_end)\d+', r'.\1', line.split(';')[0]).strip()
                if line:
                    lines.append(line)
            if name in found:
                sys.exit(f'{name}: defined twice on one side')
            found[name] = lines
    return found


def main(argv):
    if '--' not in argv:
        sys.exit(__doc__)
    cut = argv.index('--')
    old, new = kernels(argv[:cut]), kernels(argv[cut + 1:])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            verdict = 'only in ' + ('old' if name in old else 'new')
        else:
            verdict = 'same' if old[name] == new[name] else 'DIFF'
        bad += verdict != 'same'
        print(f'{verdict:12s} {len(old.get(name, new.get(name))):6d} lines  {name}')
    print(f'{len(old)} kernels old, {len(new)} kernels new, {bad} not the same')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
