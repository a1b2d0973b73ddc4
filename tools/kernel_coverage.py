#!/usr/bin/env python3
"""Which __global__ instantiations of the library did a run launch?  (A measuring aid, not a test.)

Built:    the host-side kernel handle symbols of the library (`nm` on libcineflow_hip.so or on the objects `make` leaves in csrc/).
          A handle is the data symbol that carries the kernel's own mangled name; hipcc emits one `__device_stub__` function next to
          each, which is how handles are told apart from other globals.  The mangled names are parsed here directly (`nm -C` leaves
          them mangled because of the `DF16_` parameter type): `_ZN2cf16conv_f16s_kernelILi3ELi3ELi16E...EEv...` ->
          family `cf::conv_f16s_kernel`, arguments (3, 3, 16, ...).
Launched: a rocprofv3 --kernel-trace CSV (one row per dispatch, column Kernel_Name) or a --stats CSV (columns Name, Calls); names may be
          demangled (`void cf::conv_f16s_kernel<3, 3, 16, ...>(...)`) or mangled.

Usage:  python tools/kernel_coverage.py TRACE.csv[.gz] [TRACE2.csv ...] [--lib LIB.so|OBJ.o ...] [--family REGEX] [--counts]
"""
import argparse
import csv
import gzip
import io
import os
import re
import subprocess
import sys
from collections import Counter, defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd", "cineflow", "libcineflow_hip.so")

# Itanium builtin type codes that can appear as template arguments or literal types here
_BUILTIN = {"v": "void", "b": "bool", "c": "char", "a": "signed char", "h": "unsigned char", "s": "short", "t": "unsigned short",
            "i": "int", "j": "unsigned int", "l": "long", "m": "unsigned long", "x": "long long", "y": "unsigned long long",
            "f": "float", "d": "double"}
_EXT_BUILTIN = {"DF16_": "_Float16", "DF16b": "__bf16", "Dh": "half"}


class _Unsupported(Exception):
    pass


def _source_name(s, i):
    m = re.match(r"\d+", s[i:])
    if not m:
        raise _Unsupported(s[i:])
    n = int(m.group())
    j = i + len(m.group())
    ident = s[j:j + n]
    return ("(anonymous namespace)" if ident.startswith("_GLOBAL__N") else ident), j + n


def _template_arg(s, i):
    if s[i] == "L":                                   # literal: L <type> <value> E
        j = i + 1
        for code, name in list(_EXT_BUILTIN.items()) + list(_BUILTIN.items()):
            if s.startswith(code, j):
                j += len(code)
                ty = name
                break
        else:
            raise _Unsupported(s[i:])
        k = s.index("E", j)
        raw = s[j:k]
        if ty == "bool":
            return raw == "1", k + 1
        if not re.fullmatch(r"n?\d+", raw):
            raise _Unsupported(s[i:])
        return (-int(raw[1:]) if raw.startswith("n") else int(raw)), k + 1
    for code, name in list(_EXT_BUILTIN.items()) + list(_BUILTIN.items()):
        if s.startswith(code, i):
            return name, i + len(code)
    raise _Unsupported(s[i:])


def parse_mangled(sym):
    """'_ZN2cf16conv_f16s_kernelILi3ELi3E...EEvNS_...' -> ('cf::conv_f16s_kernel', (3, 3, ...)); None when the name is no function
    (a variable) or uses a construct this small parser does not know."""
    sym = sym.split("@")[0]
    if sym.endswith(".kd"):
        sym = sym[:-3]
    if not sym.startswith("_Z") or sym.startswith("_ZZ"):
        return None
    try:
        i = 2
        parts = []
        args = ()
        if sym[i] == "N":
            i += 1
            while sym[i] != "E":
                if sym[i] == "L":                     # internal linkage marker
                    i += 1
                    continue
                if sym[i] == "I":
                    i += 1
                    out = []
                    while sym[i] != "E":
                        a, i = _template_arg(sym, i)
                        out.append(a)
                    i += 1
                    args = tuple(out)
                    continue
                name, i = _source_name(sym, i)
                parts.append(name)
            i += 1
        else:
            if sym[i] == "L":
                i += 1
            name, i = _source_name(sym, i)
            parts.append(name)
            if i < len(sym) and sym[i] == "I":
                i += 1
                out = []
                while sym[i] != "E":
                    a, i = _template_arg(sym, i)
                    out.append(a)
                i += 1
                args = tuple(out)
    except (_Unsupported, IndexError, ValueError):
        return None
    if i >= len(sym) or sym[i:].startswith("B"):      # nothing after the name: a variable, not a function
        return None
    return "::".join(parts), args


def _split_top(s, sep=","):
    out, depth, cur = [], 0, []
    for ch in s:
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        if ch == sep and depth == 0:
            out.append("".join(cur).strip())
            cur = []
        else:
            cur.append(ch)
    if cur and "".join(cur).strip():
        out.append("".join(cur).strip())
    return out


def _demangled_arg(a):
    a = a.strip()
    if a in ("true", "false"):
        return a == "true"
    m = re.fullmatch(r"\(([a-z ]+)\)(-?\d+)", a)       # (char)3, (unsigned char)1
    if m:
        a = m.group(2)
    m = re.fullmatch(r"(-?\d+)[uUlL]*", a)
    if m:
        return int(m.group(1))
    return a


def parse_demangled(name):
    """'void cf::conv_f16s_kernel<3, 3, 16, ...>(cf::ConvParams, ...)' -> ('cf::conv_f16s_kernel', (3, 3, 16, ...)); mangled names
    are handed to parse_mangled."""
    name = name.strip().strip('"')
    if name.startswith("_Z"):
        return parse_mangled(name)
    anon = "(anonymous namespace)"
    s = name.replace(anon, "\x00")
    # the qualified name ends at the first top-level '<' or '(' ; what precedes it up to the last blank is the return type
    k = len(s)
    for ch in "<(":
        p = s.find(ch)
        if p != -1:
            k = min(k, p)
    head = s[:k].split()
    if not head:
        return None
    qual = head[-1].replace("\x00", anon)
    args = ()
    if k < len(s) and s[k] == "<":
        depth, j = 0, k
        while j < len(s):
            if s[j] == "<":
                depth += 1
            elif s[j] == ">":
                depth -= 1
                if depth == 0:
                    break
            j += 1
        args = tuple(_demangled_arg(a.replace("\x00", anon)) for a in _split_top(s[k + 1:j]))
    return qual, args


def built_kernels(paths):
    """{family: set(args)} of the kernel handles in the given .so / .o files"""
    names = set()
    for path in paths:
        out = subprocess.run(["nm", path], check=True, capture_output=True, text=True).stdout
        syms = [ln.split() for ln in out.splitlines()]
        data = {f[2] for f in syms if len(f) == 3 and f[1] in "DdVvRrBbSs"}
        for f in syms:
            if len(f) >= 2 and "__device_stub__" in f[-1]:
                # _ZN2cf34__device_stub__attention_cf_kernelI... -> _ZN2cf19attention_cf_kernelI...
                h = re.sub(r"(\d+)__device_stub__", lambda m: str(int(m.group(1)) - len("__device_stub__")), f[-1], count=1)
                if h in data or not data:
                    names.add(h)
    fams = defaultdict(set)
    for n in names:
        r = parse_mangled(n)
        if r:
            fams[r[0]].add(r[1])
    return fams


def _open(path):
    if path.endswith(".gz"):
        return io.TextIOWrapper(gzip.open(path, "rb"), encoding="utf-8", newline="")
    return open(path, newline="", encoding="utf-8")


def launched_kernels(paths):
    """Counter {(family, args): dispatches} from rocprofv3 kernel-trace (Kernel_Name) or stats (Name, Calls) CSVs"""
    cnt = Counter()
    for path in paths:
        with _open(path) as f:
            rd = csv.DictReader(f)
            col = "Kernel_Name" if "Kernel_Name" in rd.fieldnames else ("Name" if "Name" in rd.fieldnames else None)
            if col is None:
                raise SystemExit("%s: no Kernel_Name / Name column" % path)
            calls = "Calls" if "Calls" in rd.fieldnames else None
            for row in rd:
                r = parse_demangled(row[col])
                if r:
                    cnt[r] += int(row[calls]) if calls else 1
    return cnt


def _fmt(args):
    return "<" + ", ".join(str(a).lower() if isinstance(a, bool) else str(a) for a in args) + ">"


def report(built, launched, family_re=None, counts=False, out=sys.stdout):
    rx = re.compile(family_re) if family_re else None
    tot_b = tot_l = 0
    for fam in sorted(built):
        if rx and not rx.search(fam):
            continue
        inst = sorted(built[fam], key=lambda a: tuple(str(x) for x in a))
        hit = [a for a in inst if launched.get((fam, a), 0) > 0]
        tot_b += len(inst)
        tot_l += len(hit)
        print("%-48s built %3d  launched %3d" % (fam, len(inst), len(hit)), file=out)
        for a in inst:
            n = launched.get((fam, a), 0)
            if n == 0:
                print("    never launched  %s%s" % (fam.split("::")[-1], _fmt(a)), file=out)
            elif counts:
                print("    %10d  %s%s" % (n, fam.split("::")[-1], _fmt(a)), file=out)
    extra = sorted(k for k in launched if k[0] in built and k[1] not in built[k[0]] and (not rx or rx.search(k[0])))
    for fam, a in extra:
        print("    launched but not in the library: %s%s" % (fam, _fmt(a)), file=out)
    print("total: %d of %d instantiations launched" % (tot_l, tot_b), file=out)
    return tot_l, tot_b


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("traces", nargs="*", help="rocprofv3 kernel_trace.csv / kernel_stats.csv files (.gz accepted)")
    ap.add_argument("--lib", nargs="+", default=[DEFAULT_LIB], help="library or objects to list the built kernels from")
    ap.add_argument("--family", help="regular expression on the qualified kernel name")
    ap.add_argument("--counts", action="store_true", help="also print the dispatch count of every launched instantiation")
    a = ap.parse_args(argv)
    report(built_kernels(a.lib), launched_kernels(a.traces), a.family, a.counts)


if __name__ == "__main__":
    main()
