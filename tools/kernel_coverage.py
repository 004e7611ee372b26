#!/usr/bin/env python3
"""Which of the compiled kernel specialisations does a run launch?

    python tools/kernel_coverage.py list [--lib LIB]
    python tools/kernel_coverage.py diff TRACE.csv [TRACE.csv | DIR ...] [--lib LIB]
                                         [--write-launched FILE]

``list`` prints every kernel instantiation of the gfx950 code object inside libgss_hip.so,
demangled, with its template arguments, one per line.  ``diff`` reads the kernel-trace CSV(s) of
a profiler run (``rocprofv3 --kernel-trace --output-format csv``: the column ``Kernel_Name``; a
directory is searched for ``*kernel_trace.csv``) and prints the instantiations that were never
launched, grouped by template; ``--write-launched FILE`` also writes the sorted names of the
library's instantiations that were launched, one per line and nothing else (the record kept as
tests/golden/kernels_launched.txt).

Host only: the code object is unbundled with clang-offload-bundler, its kernel-descriptor
symbols (``<kernel>.kd``) are read with readelf and demangled with c++filt.  Names are all this
tool reads -- it never looks at an instruction.
"""
import argparse
import csv
import os
import re
import subprocess
import sys
import tempfile
from collections import OrderedDict
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
DEFAULT_LIB = REPO / 'pb_chime5_amd' / 'lib' / 'libgss_hip.so'
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def _tool(name):
    """A binary of the ROCm LLVM toolchain (clang-offload-bundler) or of binutils."""
    roots = [os.environ.get('ROCM_PATH'), '/opt/rocm']
    for root in roots:
        if not root:
            continue
        for sub in ('lib/llvm/bin', 'llvm/bin', 'bin'):
            cand = Path(root) / sub / name
            if cand.exists():
                return str(cand)
    return name


def normalise(name):
    """One spelling per instantiation: the profiler appends '.kd' to some names, and demanglers
    differ in the return type ('void f<..>(..)'), the parameter list and blanks."""
    name = name.strip().strip('"')
    if name.endswith('.kd'):
        name = name[:-3]
    if name.endswith(' [clone .kd]'):
        name = name[:-len(' [clone .kd]')]
    name = name.replace('(anonymous namespace)::', '')
    # cut the parameter list: the first '(' at template depth 0
    depth = 0
    for i, ch in enumerate(name):
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            name = name[:i]
            break
    # drop a return type: everything up to the last blank at template depth 0
    depth = 0
    cut = 0
    for i, ch in enumerate(name):
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == ' ' and depth == 0:
            cut = i + 1
    name = name[cut:]
    name = re.sub(r'\s*,\s*', ', ', name)
    name = re.sub(r'\(\w+\)(-?\d+)', r'\1', name)           # (int)3 -> 3
    return name.strip()


def template_of(name):
    return name.split('<', 1)[0]


def _fat_binaries(lib):
    """The offload bundles of the library's .hip_fatbin section: the linker lays the fat binary
    of every translation unit one after the other, each with its own header."""
    magic = (b'__CLANG_OFFLOAD_BUNDLE__', b'CCOB')
    sections = subprocess.run(['readelf', '-SW', str(lib)], check=True, capture_output=True,
                              text=True).stdout
    m = re.search(r'\.hip_fatbin\s+\w+\s+[0-9a-f]+\s+([0-9a-f]+)\s+([0-9a-f]+)', sections)
    if not m:
        raise RuntimeError(f'{lib} has no .hip_fatbin section')
    off, size = int(m.group(1), 16), int(m.group(2), 16)
    with open(lib, 'rb') as fh:
        fh.seek(off)
        data = fh.read(size)
    starts = sorted(x.start() for mg in magic for x in re.finditer(re.escape(mg), data)
                    if x.start() % 4096 == 0)
    if not starts:
        raise RuntimeError(f'{lib}: no offload bundle in .hip_fatbin')
    return [data[a:b] for a, b in zip(starts, starts[1:] + [len(data)])]


def kernel_names(lib=DEFAULT_LIB):
    """Sorted, de-duplicated, demangled kernel instantiations of the gfx950 code object in `lib`."""
    lib = Path(lib)
    if not lib.exists():
        raise FileNotFoundError(f'{lib}: build the library first (python -m pb_chime5_amd.build)')
    mangled = OrderedDict()
    with tempfile.TemporaryDirectory() as tmp:
        for i, bundle in enumerate(_fat_binaries(lib)):
            fat, co = Path(tmp) / f'{i}.hipfb', Path(tmp) / f'{i}.co'
            fat.write_bytes(bundle)
            res = subprocess.run([_tool('clang-offload-bundler'), '--unbundle', '--type=o',
                                  f'--targets={TARGET}', f'--input={fat}', f'--output={co}'],
                                 capture_output=True, text=True)
            if res.returncode != 0 or not co.exists() or co.stat().st_size == 0:
                raise RuntimeError(f'{lib}: fat binary {i} holds no code object for {TARGET}: '
                                   f'{res.stderr.strip()}')
            syms = subprocess.run(['readelf', '-sW', str(co)], check=True, capture_output=True,
                                  text=True).stdout
            for line in syms.splitlines():
                parts = line.split()
                # Num: Value Size Type Bind Vis Ndx Name (.symtab and .dynsym both list them)
                if len(parts) >= 8 and parts[3] == 'OBJECT' and parts[7].endswith('.kd'):
                    mangled[parts[7][:-3]] = True
    if not mangled:
        return []
    out = subprocess.run(['c++filt'], input='\n'.join(mangled) + '\n', check=True,
                         capture_output=True, text=True).stdout
    return sorted({normalise(n) for n in out.splitlines() if n.strip()})


def _trace_files(paths):
    for p in map(Path, paths):
        if p.is_dir():
            yield from sorted(p.rglob('*kernel_trace.csv'))
        else:
            yield p


def launched_names(paths):
    """Normalised kernel names of every row of the kernel-trace CSV(s)."""
    seen = set()
    for path in _trace_files(paths):
        with open(path, newline='') as fh:
            reader = csv.DictReader(fh)
            col = next((c for c in (reader.fieldnames or [])
                        if c.strip().lower() in ('kernel_name', 'kernelname', 'name')), None)
            if col is None:
                raise ValueError(f'{path}: no Kernel_Name column in {reader.fieldnames}')
            for row in reader:
                if row.get(col):
                    seen.add(normalise(row[col]))
    return seen


def unreached(all_names, launched):
    """{template: [instantiations never launched]} in the order of `all_names`."""
    groups = OrderedDict()
    for name in all_names:
        if name not in launched:
            groups.setdefault(template_of(name), []).append(name)
    return groups


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    p_list = sub.add_parser('list', help='every kernel instantiation of the library')
    p_list.add_argument('--lib', default=str(DEFAULT_LIB))
    p_diff = sub.add_parser('diff', help='instantiations a traced run never launched')
    p_diff.add_argument('trace', nargs='+', help='kernel-trace CSV files or directories of them')
    p_diff.add_argument('--lib', default=str(DEFAULT_LIB))
    p_diff.add_argument('--write-launched', metavar='FILE',
                        help='write the sorted names of the launched instantiations to FILE')
    args = ap.parse_args(argv)

    names = kernel_names(args.lib)
    if args.cmd == 'list':
        for n in names:
            print(n)
        return 0
    launched = launched_names(args.trace)
    ours = set(names)
    if args.write_launched:
        Path(args.write_launched).write_text(''.join(f'{n}\n' for n in sorted(launched & ours)))
    groups = unreached(names, launched)
    missing = sum(len(v) for v in groups.values())
    print(f'{len(names)} instantiations in the library, {len(launched & ours)} launched, '
          f'{missing} never launched')
    for tmpl, members in groups.items():
        total = sum(1 for n in names if template_of(n) == tmpl)
        print(f'{tmpl}: {len(members)} of {total} never launched')
        for n in members:
            print(f'    {n}')
    foreign = sorted(launched - ours)
    if foreign:
        print(f'{len(foreign)} launched kernels are not in the library (other libraries):')
        for n in foreign:
            print(f'    {n}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
