"""Compare the gfx950 device code of two builds of csrc/, kernel by kernel (a host-only change must leave it untouched):
    python scripts/device_code_diff.py <csrc dir of build A> <csrc dir of build B>
For every *.o it dumps the .hip_fatbin section, unbundles the gfx950 code object, and compares per symbol
  - the disassembly (instruction text + encoding; the load addresses are dropped: the order in which a file's template
    instantiations are emitted follows the host code's first use of them, so a kernel's place in the file may move), and
  - the kernel's metadata record (register counts, LDS, scratch, arguments) and the bytes of its kernel descriptor.
Exit status 0 = identical."""
import os, re, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def run(*a):
    return subprocess.run(a, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    fb, co = os.path.join(tmp, "x.hipfb"), os.path.join(tmp, "x.co")
    if subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj], capture_output=True).returncode:
        return None                                                        # host-only file
    run(LLVM + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co, "--unbundle")
    return co


def symbols(co):
    """{symbol: text}: functions from the disassembly, 'meta:<kernel>' records from the notes, '<kernel>.kd' descriptor bytes."""
    out, cur = {}, None
    for line in run(LLVM + "/llvm-objdump", "-d", "--no-leading-addr", co).splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and line.strip() not in ("", "..."):                        # "...": zero padding behind the section's last function
            out[cur].append(re.sub(r"// [0-9A-F]+:", "//", line))            # keep the encoding, drop the address
    cur = None
    for line in run(LLVM + "/llvm-readelf", "--notes", co).splitlines():
        if not line.startswith(" "):                                         # amdhsa.kernels: / amdhsa.target: ...
            cur = None
        if line.startswith("  - ."):                                         # one record per kernel; .name comes inside it
            cur = []
            out["meta:%d" % len(out)] = cur
        if cur is not None:
            cur.append(line)
    named = {}
    for k, v in out.items():
        if k.startswith("meta:"):
            name = [l.split(":", 1)[1].strip() for l in v if l.strip().startswith(".name:")]
            if name:
                named["meta:" + name[0]] = v
        else:
            named[k] = v
    sec = re.search(r"\] \.rodata\s+\S+\s+([0-9a-f]+) ([0-9a-f]+) ", run(LLVM + "/llvm-readelf", "-S", "-W", co))
    raw = open(co, "rb").read()
    for line in run(LLVM + "/llvm-objdump", "--syms", co).splitlines():
        m = re.match(r"^([0-9a-f]+) .* \.rodata\s+([0-9a-f]+)\s+(?:\.\w+\s+)?(\S+\.kd)$", line)
        if m and sec:
            at = int(sec.group(2), 16) + int(m.group(1), 16) - int(sec.group(1), 16)
            d = bytearray(raw[at:at + int(m.group(2), 16)])
            d[16:24] = bytes(8)                                              # the entry offset is relative to the descriptor's place
            named[m.group(3)] = [d.hex()]
    nmeta, nkd = sum(k.startswith("meta:") for k in named), sum(k.endswith(".kd") for k in named)
    if nmeta != nkd:
        sys.exit("%s: %d metadata records for %d kernel descriptors (llvm-readelf's notes format changed?)" % (co, nmeta, nkd))
    return named


def main(a, b):
    bad = 0
    for f in sorted(os.listdir(a)):
        if not f.endswith(".o"):
            continue
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            ca, cb = code_object(os.path.join(a, f), ta), code_object(os.path.join(b, f), tb)
            if ca is None or cb is None:
                print("%-16s no device code%s" % (f, "" if ca is cb else "  IN ONE BUILD ONLY"))
                bad += ca is not cb
                continue
            same_file = open(ca, "rb").read() == open(cb, "rb").read()
            sa, sb = symbols(ca), symbols(cb)
        diff = sorted(k for k in set(sa) | set(sb) if sa.get(k) != sb.get(k))
        nk = sum(k.endswith(".kd") for k in sa)
        print("%-16s %3d kernels, %4d symbols compared: %s%s" % (f, nk, len(sa), "DIFFER" if diff else "identical",
                                                                  " (code object byte-identical)" if same_file else ""))
        for k in diff:
            print("    differs: " + k)
        bad += len(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
