#!/usr/bin/env python3
"""Per-kernel hashes of device assembly, and their comparison across a code move.

Input: assembly files from
    hipcc <FLAGS of kaldi-lstm_amd/build.py> --cuda-device-only -S -cuid=<fixed> <source>.hip -o <source>.s
Moving a kernel changes its position in its file and local labels carry that position (.LBB<f>_<n>, .Lfunc_end<f>), so
files are compared per kernel (the rule of profiles/kernels_split_isa.txt, "command"):
  * lines that begin with ';', .file, .loc or .ident are dropped, and so are trailing ';' comments;
  * a kernel's text runs from its .protected line through its .amdhsa_kernel ... .end_amdhsa_kernel block to its .size line;
  * the <f> of .LBB<f>_<n> and .Lfunc_end<f> is replaced by a constant;
  * sha256 per kernel text, and per kernel entry of amdhsa.kernels in .amdgpu_metadata (registers, LDS, scratch,
    argument layout);
  * per file (or any group of kernels): sha256 over the sorted per-kernel hashes, joined by newlines.

    kernel_isa_hash.py a.s [b.s ...]                           list kernels and hashes per file
    kernel_isa_hash.py --before old.s [..] --after new.s [..]  compare; exit status 1 if a symbol is lost, added,
                                                               present in two files of a set, or differs

It hashes and compares text; it does not look at what the instructions are."""
import argparse
import hashlib
import os
import re
import sys

_DROP = re.compile(r"^\s*(;|\.file\b|\.loc\b|\.ident\b)")
_LABEL = re.compile(r"\.(LBB|Lfunc_end)\d+")
_PROTECTED = re.compile(r"^\s*\.protected\s+(\S+)")
_SIZE = re.compile(r"^\s*\.size\s+(\S+)\s*,")
_END_KERNEL = re.compile(r"^\s*\.end_amdhsa_kernel\b")
_MD_NAME = re.compile(r"^(?:    |  - )\.name:\s+(\S+)")


def _sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def _strip_comment(line):
    """The line up to its first ';' that is not inside a quoted string (.ascii / .asciz text, section names)."""
    quoted = False
    i = 0
    while i < len(line):
        c = line[i]
        if quoted and c == "\\":
            i += 1                                       # (the escaped character, a quote included, belongs to the string)
        elif c == '"':
            quoted = not quoted
        elif c == ";" and not quoted:
            return line[:i]
        i += 1
    return line


def clean(text):
    """The lines that count: no comments, no debug-location or producer lines, no trailing blanks."""
    out = []
    for line in text.splitlines():
        if _DROP.match(line):
            continue
        line = _strip_comment(line).rstrip()
        if line:
            out.append(line)
    return out


def kernel_hashes(text):
    """{kernel symbol: (text sha256, metadata sha256)} of one assembly file."""
    lines = clean(text)
    texts, i = {}, 0
    while i < len(lines):
        m = _PROTECTED.match(lines[i])
        if not m:
            i += 1
            continue
        sym, j, closed = m.group(1), i, False
        while j < len(lines):                            # ... through the kernel descriptor to the .size line behind it
            if _END_KERNEL.match(lines[j]):
                closed = True
            s = _SIZE.match(lines[j])
            if closed and s and s.group(1) == sym:
                break
            j += 1
        if j == len(lines):
            raise ValueError("kernel %s: no .size line behind its .end_amdhsa_kernel" % sym)
        if sym in texts:
            raise ValueError("kernel %s: twice in one file" % sym)
        texts[sym] = _sha([_LABEL.sub(r".\g<1>F", l) for l in lines[i:j + 1]])
        i = j + 1
    meta = _metadata_hashes(lines)
    if set(meta) != set(texts):
        raise ValueError("kernels with text and kernels with metadata differ: %s" % sorted(set(meta) ^ set(texts)))
    return {sym: (texts[sym], meta[sym]) for sym in texts}


def _metadata_hashes(lines):
    """sha256 of every entry of amdhsa.kernels: an entry opens with '  - .<key>:' at the list's indent and runs to the next one."""
    try:
        k = next(n for n, l in enumerate(lines) if l.strip() == "amdhsa.kernels:")
    except StopIteration:
        return {}
    entries, cur = [], None
    for l in lines[k + 1:]:
        if re.match(r"^  - \.", l):
            cur = [l]
            entries.append(cur)
        elif l.startswith("    ") and cur is not None:
            cur.append(l)
        else:
            break                                        # the next top-level key (amdhsa.target, ...) or the end marker
    out = {}
    for e in entries:
        names = [m.group(1) for m in map(_MD_NAME.match, e) if m]       # (an argument's .name sits deeper)
        if len(names) != 1:
            raise ValueError("metadata entry with %d kernel names" % len(names))
        out[names[0]] = _sha(e)
    return out


def group_hash(hashes):
    """sha256 over the sorted hashes, joined by newlines."""
    return hashlib.sha256("\n".join(sorted(hashes)).encode()).hexdigest()


def load(paths):
    """[(path, {symbol: (text, metadata)})] and the symbols that sit in more than one of the files."""
    files, seen, dup = [], {}, set()
    for p in paths:
        with open(p) as fh:
            h = kernel_hashes(fh.read())
        for sym in h:
            if sym in seen:
                dup.add(sym)
            seen[sym] = p
        files.append((p, h))
    return files, sorted(dup)


def merged(files):
    out = {}
    for _, h in files:
        out.update(h)
    return out


def compare(before, after):
    """before, after: lists of (path, hashes).  Returns (lost, added, in_two, differing) symbol lists."""
    b, a = merged(before), merged(after)
    in_two = sorted({s for fs in (before, after) for n, (_, h) in enumerate(fs) for s in h if any(s in g for _, g in fs[n + 1:])})
    return sorted(set(b) - set(a)), sorted(set(a) - set(b)), in_two, sorted(s for s in b if s in a and b[s] != a[s])


def _print_files(files, verbose):
    for p, h in files:
        print("%s  %d kernels  text %s  metadata %s" % (p, len(h), group_hash(t for t, _ in h.values()), group_hash(m for _, m in h.values())))
        if verbose:
            for sym in sorted(h):
                print("    %s  %s  %s" % (h[sym][0], h[sym][1], sym))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="*", help="assembly files to list")
    ap.add_argument("--before", nargs="+", default=[])
    ap.add_argument("--after", nargs="+", default=[])
    ap.add_argument("-v", "--verbose", action="store_true", help="one line per kernel")
    ap.add_argument("--group", action="append", default=[], metavar="NAME=PART[,PART...]",
                    help="also print the hash pair of a group of kernels of the 'after' set (or of the listed files): a PART is "
                         "@FILE (every kernel of that assembly file, by base name) or a regular expression a symbol must match")
    a = ap.parse_args(argv)
    if bool(a.before) != bool(a.after) or (a.files and a.before) or not (a.files or a.before):
        ap.error("give files to list, or --before and --after")
    bad = 0
    if a.files:
        files, dup = load(a.files)
        _print_files(files, a.verbose)
        if dup:
            print("in two files: %s" % " ".join(dup))
            bad = 1
        pool, pool_files = merged(files), files
    else:
        before, _ = load(a.before)
        after, _ = load(a.after)
        print("before:")
        _print_files(before, a.verbose)
        print("after:")
        _print_files(after, a.verbose)
        lost, added, in_two, differing = compare(before, after)
        nb, na = len(merged(before)), len(merged(after))
        print("%d kernel symbols before, %d after: %d lost, %d added, %d in two files, %d differing"
              % (nb, na, len(lost), len(added), len(in_two), len(differing)))
        for what, syms in (("lost", lost), ("added", added), ("in two files", in_two), ("differs", differing)):
            for s in syms:
                print("  %s: %s" % (what, s))
        bad = 1 if lost or added or in_two or differing else 0
        pool, pool_files = merged(after), after
        if not bad:
            print("every kernel's text EQUAL, every metadata entry EQUAL")
            b = merged(before)
            print("all  %d  text %s  metadata %s" % (len(b), group_hash(t for t, _ in b.values()), group_hash(m for _, m in b.values())))
    for g in a.group:
        name, parts = g.split("=", 1)
        syms = set()
        for part in parts.split(","):
            if part.startswith("@"):
                hit = [h for p, h in pool_files if os.path.basename(p) == part[1:]]
                if len(hit) != 1:
                    ap.error("group %s: %s names %d of the files" % (name, part, len(hit)))
                syms |= set(hit[0])
            else:
                syms |= {s for s in pool if re.search(part, s)}
        sel = [pool[s] for s in syms]
        print("group %s  %d kernels  text %s  metadata %s" % (name, len(sel), group_hash(t for t, _ in sel), group_hash(m for _, m in sel)))
    return bad


if __name__ == "__main__":
    sys.exit(main())
