'''Compares the kernels of two device-assembly listings of one source file (hipcc <CXXFLAGS of csrc/Makefile> -S
--cuda-device-only), kernel by kernel: identical or different after stripping comments and directives, replacing mangled
symbols and renumbering .LBB labels; instruction counts, VGPRs, SGPRs, scratch and LDS bytes of both sides.

    python tools/isa_compare.py old.s new.s [--rename REGEX REPL]... > profiles/<name>.txt

--rename rewrites a NEW kernel's demangled name into the name of its counterpart in the old listing, e.g.
    --rename 'k_attention_w8<(.*), 2>' 'k_attention_w8q2<\\1>' --rename 'k_attention_w8<(.*), 1>' 'k_attention_w8<\\1>'
Exit status 1 when a kernel has no counterpart.'''
import argparse
import re
import subprocess
import sys

RES = {'vgpr': 'NumVgprs', 'sgpr': 'TotalNumSgprs', 'scratch': 'ScratchSize', 'lds': 'LDSByteSize'}


def kernels(path):
    '''demangled name -> (normalised instruction lines, {vgpr, sgpr, scratch, lds}).'''
    lines = open(path, encoding='utf-8').read().split('\n')
    syms = [m.group(1) for ln in lines for m in [re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln)] if m]
    names = subprocess.run(['c++filt'] + syms, capture_output=True, text=True, check=True).stdout.split('\n')
    out = {}
    for sym, name in zip(syms, names):
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ':'))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
        labels, body = {}, []
        for ln in lines[start + 1:end]:
            ln = ln.split(';')[0].strip()
            if not ln or (ln.startswith('.') and not ln.endswith(':')):
                continue
            ln = re.sub(r'\b_Z\w+', 'SYM', ln)
            ln = re.sub(r'\.LBB\d+_\d+', lambda m: labels.setdefault(m.group(0), '.L%d' % len(labels)), ln)
            body.append(ln)
        res = {}
        for ln in lines[end:end + 80]:
            for key, tag in RES.items():
                m = re.match(r';\s*%s:\s*(\d+)' % tag, ln)
                if m and key not in res:
                    res[key] = int(m.group(1))
        out[re.sub(r'^void |\(AttnArgs\)$', '', name)] = (body, res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--rename', nargs=2, action='append', default=[], metavar=('REGEX', 'REPL'))
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    print('# kernel (new name) | verdict | instructions old/new | VGPR old/new | SGPR old/new | scratch bytes old/new | LDS bytes old/new')
    missing, seen = [], set()
    for name in sorted(new):
        was = name
        for pat, repl in args.rename:
            was = re.sub(pat, repl, was)
        if was not in old:
            missing.append(name)
            continue
        seen.add(was)
        (ob, orr), (nb, nr) = old[was], new[name]
        same = ob == nb and orr == nr
        cols = ['%d/%d' % (len([l for l in ob if not l.endswith(':')]), len([l for l in nb if not l.endswith(':')]))]
        cols += ['%d/%d' % (orr[k], nr[k]) for k in ('vgpr', 'sgpr', 'scratch', 'lds')]
        print('%-48s | %s | %s%s' % (name, 'identical' if same else 'DIFFERENT', ' | '.join(cols),
                                     '' if was == name else '   (was %s)' % was))
    missing += ['(old) ' + n for n in sorted(set(old) - seen)]
    for n in missing:
        print('no counterpart: ' + n)
    return 1 if missing else 0


if __name__ == '__main__':
    sys.exit(main())
