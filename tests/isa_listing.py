"""gfx950 assembly listings of the kernel sources, made and cut in one place.

The ISA tests (test_isa_waits.py, test_isa_waits_hi.py, test_isa_store_hazard.py) and the tools
(tools/isa_identity.py, tools/isa_count.py) read what hipcc emits for a source of e-raft_amd/csrc.
The compile command is the one `make` itself would run for that source's object, turned from `-c`
into a device-only `-S`: common flags, per-object `FLAGS +=` and HIPCC / ARCH overrides are the
Makefile's by construction, in this tree or in any other copy of csrc (a worktree of the parent
commit, a patched scratch copy) that sits beside its ../../include.  CPU only.
"""
import collections
import concurrent.futures
import functools
import os
import re
import shlex
import subprocess


def sources(csrc):
    """The Makefile's SRCS (the only read of the Makefile's text; flags come from make itself)."""
    with open(os.path.join(csrc, "Makefile")) as f:
        m = re.search(r"^SRCS\s*:=\s*(.*)$", f.read(), re.M)
    assert m, f"no SRCS in {csrc}/Makefile"
    return m.group(1).split()


def object_command(csrc, src):
    """argv of the compile line `make` prints for build/<name>.o (a dry run: nothing is built)."""
    obj = "build/" + src[:-len(".hip")] + ".o"
    out = subprocess.run(["make", "-n", "-B", "--no-print-directory", "-C", csrc, obj],
                         check=True, capture_output=True, text=True).stdout
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" in argv and src in argv and argv[-2:] == ["-o", obj]:
            return argv
    raise AssertionError(f"make -n {obj} in {csrc} prints no compile line:\n{out}")


def compile_command(csrc, src, out="-"):
    """argv (to run in csrc) that compiles src's device code to assembly with its object's flags."""
    argv = object_command(csrc, src)
    i = argv.index("-c")
    return argv[:i] + ["--cuda-device-only", "-S"] + argv[i + 1:-1] + [out]


@functools.lru_cache(maxsize=None)
def _listing(csrc, src):
    return subprocess.run(compile_command(csrc, src), cwd=csrc, check=True, capture_output=True, text=True).stdout


def listing(csrc, src):
    """The assembly text of csrc/src; compiled once per process and (tree, source)."""
    return _listing(os.path.realpath(csrc), src)


def compile_all(csrc, srcs=None):
    """{source: listing} of srcs (default: all of SRCS), compiled in a thread pool of at most 8."""
    srcs = list(srcs or sources(csrc))
    with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(srcs, ex.map(lambda s: listing(csrc, s), srcs)))


def instructions(lines):
    """The instruction lines among a listing's lines: tab-led, no directives, comments or label
    definitions; trailing `;` comments cut, the function index of local labels `.LBB<n>_` dropped
    (a kernel added earlier in the file shifts it)."""
    return [re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()) for ln in lines
            if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]


class Kernel(collections.namedtuple("Kernel", "name body ins desc meta occupancy")):
    """One kernel of a listing: its mangled name, the raw lines of its body (label definitions and
    comments included), its instruction lines, the numbers of its `.amdhsa_` descriptor (desc:
    next_free_vgpr, group_segment_fixed_size, ...) and of its amdhsa.kernels metadata record (meta:
    vgpr_count, vgpr_spill_count, sgpr_spill_count, max_flat_workgroup_size, ...), and the compiler's
    `; Occupancy:` line (waves per SIMD)."""
    __slots__ = ()
    vgpr = property(lambda k: k.desc["next_free_vgpr"])             # arch + acc, as allocated
    lds = property(lambda k: k.desc["group_segment_fixed_size"])
    scratch = property(lambda k: k.desc["private_segment_fixed_size"])


@functools.lru_cache(maxsize=None)
def kernels(text):
    """{mangled name: Kernel} of a listing (device functions that are no kernels are left out)."""
    records = re.split(r"\n  - (?=\.)", text[text.index("amdhsa.kernels:"):])
    meta = {re.search(r"^ *\.name:\s+(\S+)$", r, re.M).group(1):
            {k: int(v) for k, v in re.findall(r"^(?:    )?\.(\w+):\s+(\d+)$", r, re.M)} for r in records[1:]}
    res = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        name, desc = m.group(1), m.group(2)
        start = re.search("^" + re.escape(name) + ":", text, re.M).start()
        end = text.index(".Lfunc_end", start)
        body = text[start:end].splitlines()
        res[name] = Kernel(name, body, instructions(body),
                           {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", desc)}, meta[name],
                           int(re.compile(r"^; Occupancy: (\d+)", re.M).search(text, end).group(1)))
    return res


def find(text, fragment):
    """The one kernel of the listing whose mangled name contains `fragment`."""
    hits = [k for name, k in kernels(text).items() if fragment in name]
    assert len(hits) == 1, f"{fragment}: {len(hits)} kernels match ({[k.name for k in hits] or 'none in the listing'})"
    return hits[0]
