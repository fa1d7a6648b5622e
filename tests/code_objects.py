"""The gfx950 code objects inside a built library (no GPU): their kernel descriptors, and the template arguments of
the decode GEMV and GEMM-prefill kernels read straight from the Itanium-mangled kernel names.

Reads the .hip_fatbin section with the LLVM tools of the ROCm install.  Used by test_code_objects.py (no kernel may
use scratch), by the coverage gates (every compiled instantiation is launched: test_decode_instantiations_gpu.py,
test_prefill_gemm_instantiations_gpu.py, test_attention_instantiations_gpu.py,
test_prompt_attention_instantiations_gpu.py, test_cls_screen_instantiations_gpu.py,
test_gemm16_gpu.py and, through wcopy_cases.coverage_gate, the five weight-copy modules), by the CPU modules that pin
a feature's compiled kernel set (test_w16_pass.py, test_w16_f16.py, test_q4.py, test_gemm16.py, test_seq_gemm.py) and
by the GPU modules that look a launched kernel up (test_seq_*_gpu.py, test_cls_screen_q8_gpu.py)."""
import os
import re
import shutil
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def tools_present():
    return all(os.path.exists(t) for t in TOOLS)


def code_object_notes(lib):
    """`llvm-readelf --notes` of every gfx950 code object bundled into the shared library `lib`, concatenated."""
    td = tempfile.mkdtemp(prefix="kh_co_")
    try:
        fat = os.path.join(td, "fat.bin")
        subprocess.check_call([TOOLS[0], "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        assert starts, "no offload bundle in .hip_fatbin"
        notes = []
        for i, s in enumerate(starts):
            chunk = os.path.join(td, f"bundle{i}.bin")
            with open(chunk, "wb") as f:
                f.write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            co = os.path.join(td, f"co{i}.elf")
            subprocess.check_call([TOOLS[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   f"--input={chunk}", f"--output={co}"], stderr=subprocess.DEVNULL)
            if os.path.getsize(co) == 0:
                continue  # a translation unit without device code
            notes.append(subprocess.check_output([TOOLS[2], "--notes", co], text=True))
        return "\n".join(notes)
    finally:
        shutil.rmtree(td, ignore_errors=True)


def kernel_scratch(notes):
    """{mangled kernel name: private segment (scratch) bytes} from code_object_notes()."""
    kernels = {}
    name = None
    for line in notes.splitlines():
        m = re.search(r"\.name:\s+(\S+)", line)
        if m and m.group(1).startswith("_Z"):
            name = m.group(1)
        m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", line)
        if m:
            kernels.setdefault(name or f"?{len(kernels)}", int(m.group(1)))
            name = None
    return kernels


# _Z<len><name>I<args>E...: a kernel template instantiation.  Its leading literal arguments are Lb0E / Lb1E (bool)
# and Li<n>E / Lin<n>E (int, n: negative); a class argument ends the literal run.  _ZL<len><name>...: a kernel with
# internal linkage (static).
_MANGLED = re.compile(r"^_Z(\d+)")
_PLAIN = re.compile(r"^_ZL?(\d+)")
_LITERAL = re.compile(r"L([bi])(n?)(\d+)E")


def template_name(mangled):
    """'_Z5k_qkvILb0ELi2ELi0ELi1EEv9KhQkvArgs' -> 'k_qkv<false,2,0,1>' (the leading literal template arguments);
    None for a name that is not a template instantiation."""
    m = _MANGLED.match(mangled)
    if not m:
        return None
    n = int(m.group(1))
    p = m.end() + n
    stem = mangled[m.end():p]
    if mangled[p:p + 1] != "I":
        return None
    p += 1
    args = []
    while True:
        a = _LITERAL.match(mangled, p)
        if not a:
            break
        v = int(a.group(3)) * (-1 if a.group(2) else 1)
        args.append(("true" if v else "false") if a.group(1) == "b" else str(v))
        p = a.end()
    return f"{stem}<{','.join(args)}>"


def plain_name(mangled):
    """'_ZL9k_pg_ropePfS_PKfS1_iiiii' -> 'k_pg_rope' (a kernel that is not a template, static or not); None for a
    template instantiation or a name that is not mangled."""
    m = _PLAIN.match(mangled)
    if not m:
        return None
    p = m.end() + int(m.group(1))
    return None if mangled[p:p + 1] == "I" else mangled[m.end():p]


def instantiations(notes, stems):
    """Distinct template_name()s of the kernels in code_object_notes() whose name is one of `stems`."""
    out = set()
    for k in kernel_scratch(notes):
        t = template_name(k)
        if t and t.split("<")[0] in stems:
            out.add(t)
    return out


def kernels(notes, stems):
    """instantiations() plus the plain_name()s of the non-template kernels whose name is one of `stems`."""
    out = instantiations(notes, stems)
    for k in kernel_scratch(notes):
        n = plain_name(k)
        if n in stems:
            out.add(n)
    return out
