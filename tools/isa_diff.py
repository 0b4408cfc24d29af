"""Do two builds hold the same kernels?  Compares the device assembly the build keeps under NFI_KEEP_ASM=1, by kernel name:

    python tools/isa_diff.py OLD.s [OLD.s ...] -- NEW.s [NEW.s ...]        # e.g. build/*.legal.s of two trees

Each file is cut into functions (from a function's label to its .Lfunc_end, the .amdhsa_ descriptor block included);
comments go, and the label counters that depend on a function's place in its file (.LBB<n>_, .Ltmp<n>, .Lfunc_end<n>)
are normalised.  What is left - instruction text and descriptor - is compared as text.  Prints each side's kernel count
and every missing, extra or differing function; exit status 1 if there is one.  Which file a function sits in, and
where, is not compared: moving kernels between translation units is exactly what this is meant to let through."""
import re
import sys

FUNC_TYPE = re.compile(r'^\s*\.type\s+(\S+),@function')
LABEL = re.compile(r'^([A-Za-z_$][\w$.]*):')
COUNTER = re.compile(r'\.L(BB|func_end|func_begin)\d+')
TMP = re.compile(r'\.Ltmp\d+')


def functions(text):
    """{name: (normalised text, is a kernel)} of one assembly file."""
    out, names, name, body = {}, set(), None, []
    for line in text.splitlines():
        line = line.split(';', 1)[0].rstrip()
        m = FUNC_TYPE.match(line)
        if m:
            names.add(m.group(1))
        m = LABEL.match(line)
        if name is None and m and m.group(1) in names:
            name, body = m.group(1), []
        if name is None or not line.strip():
            continue
        body.append(COUNTER.sub(lambda c: '.L' + c.group(1), line))
        if line.startswith('.Lfunc_end'):
            tmps = {}
            joined = TMP.sub(lambda t: '.Ltmp_%d' % tmps.setdefault(t.group(0), len(tmps)), '\n'.join(body))
            assert name not in out, 'defined twice in one file: ' + name
            out[name] = (joined, '.amdhsa_kernel' in joined)
            name = None
    return out


def side(paths):
    funcs = {}
    for p in paths:
        for name, f in functions(open(p).read()).items():
            assert name not in funcs, 'defined in two files: ' + name
            funcs[name] = f
    return funcs


def diff(old, new):
    """Report lines for two {name: (text, is_kernel)} maps, empty when they agree."""
    lines = ['missing (old side only): ' + n for n in sorted(set(old) - set(new))]
    lines += ['extra (new side only): ' + n for n in sorted(set(new) - set(old))]
    lines += ['differs: ' + n for n in sorted(set(old) & set(new)) if old[n] != new[n]]
    return lines


def main(argv):
    if '--' not in argv or argv[0] == '--' or argv[-1] == '--':
        sys.exit(__doc__)
    cut = argv.index('--')
    old, new = side(argv[:cut]), side(argv[cut + 1:])
    for label, funcs in (('old', old), ('new', new)):
        print('%s: %d kernels, %d functions in all' % (label, sum(k for _, k in funcs.values()), len(funcs)))
    report = diff(old, new)
    print('\n'.join(report) if report else 'the same on both sides')
    return 1 if report else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
