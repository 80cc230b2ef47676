#!/usr/bin/env python3
"""Generate dora-gpu-sys/src/ffi.rs (Rust `extern "C"` declarations) from include/dora_gpu.h.

    python integration/rust/gen_ffi.py        # rewrites the file; tests/test_rust_binding.py
                                              # checks that it matches the header
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(ROOT, "include", "dora_gpu.h")
OUT = os.path.join(ROOT, "integration", "rust", "dora-gpu-sys", "src", "ffi.rs")

TICKET_HEADER = os.path.join(ROOT, "include", "dora_fill_ticket.h")

OPAQUE = {"dora_plan", "dora_node", "dora_sample", "dora_event", "dora_daemon"}
# structs passed by pointer that the caller allocates: declared here as opaque #[repr(C)] blocks
# of the size their header states (dora_fill_ticket.h: DORA_FILL_TICKET_SIZE)
SIZED = {"dora_fill_ticket"}
# plain structs the caller fills in, declared field by field from the header (struct_decl)
STRUCTS = {"dora_tensor", "dora_tensor_cast", "dora_tensor_quant", "dora_tensor_field",
           "dora_tensor_list",
           "dora_tensor_take", "dora_tensor_mask", "dora_tensor_affine", "dora_tensor_reduce",
           "dora_tensor_resize", "dora_tensor_crop", "dora_tensor_prep"}
SCALAR = {"uint16_t": "u16", "int": "c_int", "int64_t": "i64", "uint64_t": "u64", "uint32_t": "u32",
          "int32_t": "i32", "size_t": "usize", "float": "f32", "double": "f64",
          "uint8_t": "u8", "char": "c_char", "void": "c_void", "ArrowDeviceType": "ArrowDeviceType",
          "dora_stream_t": "dora_stream_t", "dora_event_t": "dora_event_t",
          "struct ArrowArray": "ArrowArray", "struct ArrowSchema": "ArrowSchema"}


def prototypes(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#[^\n]*", "", text)
    text = re.sub(r"struct\s+Arrow\w+\s*\{.*?\};", "", text, flags=re.S)
    text = re.sub(r"enum\s*\{.*?\};", "", text, flags=re.S)
    text = re.sub(r"typedef[^;]*;", "", text)
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(dora_\w+)\s*\(([^)]*)\)\s*;", text):
        yield " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())


def rust_type(c):
    c = c.strip()
    stars = c.count("*")
    base = c.replace("*", " ").split()
    consts = [i for i, w in enumerate(c.replace("*", " * ").split()) if w == "const"]
    words = [w for w in base if w != "const"]
    name = " ".join(words)
    if name in OPAQUE or name in SIZED or name in STRUCTS:
        t = name
    elif name in SCALAR:
        t = SCALAR[name]
    else:
        raise SystemExit(f"unmapped C type: {c!r}")
    # pointer levels: the outermost pointer is const when `const` follows the last `*`
    toks = c.replace("*", " * ").split()
    levels = []
    prev_const = toks[0] == "const" or (len(toks) > 1 and toks[1] == "const" and toks[0] != "*")
    const_of_pointee = toks[0] == "const" or (name in SCALAR and "const" in toks[:toks.index("*")] if "*" in toks else False)
    # walk: after each '*', a following 'const' qualifies that pointer itself (rare here)
    ptr_consts = []
    for i, w in enumerate(toks):
        if w == "*":
            ptr_consts.append(i + 1 < len(toks) and toks[i + 1] == "const")
    pointee_const = "const" in toks[:toks.index("*")] if "*" in toks else False
    for k in range(stars):
        # innermost pointer points at the base type; its constness is pointee_const; outer
        # pointers point at pointers whose constness is ptr_consts of the previous level
        is_const = pointee_const if k == 0 else ptr_consts[k - 1]
        t = f"*{'const' if is_const else 'mut'} {t}"
    return t


def param_list(args):
    if args.strip() in ("", "void"):
        return []
    out = []
    for i, a in enumerate(args.split(",")):
        a = a.strip()
        m = re.match(r"(.*?)(\b\w+)$", a)
        ctype, pname = m.group(1), m.group(2)
        if not ctype.strip() or ctype.strip().endswith(("struct", "const")):
            ctype, pname = a, f"arg{i}"
        pname = {"type": "type_", "ref": "ref_", "in": "in_", "fn": "fn_"}.get(pname, pname)
        out.append((pname, rust_type(ctype)))
    return out


def ticket_decl():
    """dora_fill_ticket as an opaque block of the size its header states (a kernel argument the
    Rust side only carries), and the header's mode constants."""
    text = open(TICKET_HEADER).read()
    size = int(re.search(r"#define\s+DORA_FILL_TICKET_SIZE\s+(\d+)", text).group(1))
    assert size % 8 == 0, size
    out = [f"/// `dora_fill_ticket` (include/dora_fill_ticket.h): {size} bytes, 8-byte aligned; passed by",
           "/// value to the kernel that publishes the sample.",
           "#[repr(C)]", "#[derive(Clone, Copy, Default)]",
           "pub struct dora_fill_ticket {", f"    _opaque: [u64; {size // 8}],", "}"]
    for name in ("DORA_FILL_WRITE_THROUGH", "DORA_FILL_PLAIN", "DORA_FILL_MAX_WORKGROUPS"):
        v = re.search(rf"#define\s+{name}\s+(\d+)u?\b", text).group(1)
        out.append(f"pub const {name}: u32 = {v};")
    return out


def struct_decl(name, text):
    """A plain struct of the header as a #[repr(C)] Rust struct with the same fields in the same
    order, each type mapped as a parameter's would be (tests/test_rust_binding.py holds ffi.rs to
    this generator's output, so a header edit that is not regenerated fails there)."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S)
    if not m:
        raise SystemExit(f"struct {name} not found in the header")
    out = [f"/// `{name}` (include/dora_gpu.h), field for field.",
           "#[repr(C)]", "#[derive(Clone, Copy)]", f"pub struct {name} {{"]
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        first, *more = [d.strip() for d in decl.split(",")]  # (`float a, b`: members of one type)
        fm = re.match(r"(.*?)(\b\w+)(?:\[(\d+)\])?$", first)
        t = rust_type(fm.group(1))
        for member in [fm.group(2) + (f"[{fm.group(3)}]" if fm.group(3) else ""), *more]:
            mm = re.match(r"(\w+)(?:\[(\d+)\])?$", member)
            # (a fixed array member)
            out.append(f"    pub {mm.group(1)}: {f'[{t}; {mm.group(2)}]' if mm.group(2) else t},")
    out.append("}")
    return out


def main():
    lines = ["// Generated by integration/rust/gen_ffi.py from include/dora_gpu.h -- do not edit.",
             "// tests/test_rust_binding.py checks that every function of the header is declared",
             "// here with the same parameter count.",
             "use crate::*;", "use std::os::raw::{c_char, c_int, c_void};", "",
             *ticket_decl(), "",
             *[ln for n in sorted(STRUCTS) for ln in struct_decl(n, open(HEADER).read())], "",
             'extern "C" {']
    for ret, name, args in prototypes(open(HEADER).read()):
        ps = ", ".join(f"{n}: {t}" for n, t in param_list(args))
        r = rust_type(ret)
        tail = "" if r == "c_void" else f" -> {r}"
        lines.append(f"    pub fn {name}({ps}){tail};")
    lines.append("}")
    src = "\n".join(lines) + "\n"
    if "--check" in sys.argv:
        sys.exit(0 if open(OUT).read() == src else 1)
    open(OUT, "w").write(src)


if __name__ == "__main__":
    main()
