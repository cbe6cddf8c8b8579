"""Per-kernel register / LDS / scratch usage of a built object (parallelwavegan_amd/csrc/build/<name>.hip.o).

Usage: python tools/kernel_resources.py conv1d [conv1d_wgrad ...]
       python tools/kernel_resources.py --compare OTHER_BUILD_DIR conv1d_wgrad [gconv ...]
Reads the gfx950 code object out of the object's .hip_fatbin section and prints the AMDGPU metadata notes:
kernel name, VGPRs, AGPRs, SGPRs, spilled VGPRs / SGPRs, scratch bytes, static LDS.  Used to check that an edit of
a hot kernel did not change its register allocation (hipcc's allocation for the 2x2-tile convolution waves flips
between 174 and 256 VGPRs on unrelated edits, csrc/conv1d.hip).

--compare: is the device code of this tree's object the same as that of the object of the same name under OTHER_BUILD_DIR
(another checkout's csrc/build), kernel by kernel?  Hashes every FUNC symbol's bytes of the gfx950 code object (taken from
its section by the symbol's address and size) and compares the sets of names and the hashes; prints the kernel count and,
for every kernel that differs, both resource lines.  Exit status 1 if anything differs.  Per kernel and not the whole code
object: two builds of one source in different directories agree in every kernel's bytes but not in the object's hash.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unbundle(obj, d):
    """The gfx950 code object of ``obj``, written into directory ``d``."""
    fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    return co


def kernel_hashes(obj):
    """{mangled name: sha256 of the function's bytes} over the FUNC symbols of the object's gfx950 code object."""
    with tempfile.TemporaryDirectory() as d:
        co = unbundle(obj, d)
        image = open(co, "rb").read()
        sections = {}  # index -> (address, file offset)
        for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S+\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)",
                             subprocess.check_output([f"{LLVM}/llvm-readelf", "-S", "-W", co], text=True), re.M):
            sections[m[1]] = (int(m[2], 16), int(m[3], 16))
        symbols = subprocess.check_output([f"{LLVM}/llvm-readelf", "--symbols", "-W", co], text=True)
    out = {}
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", symbols, re.M):
        addr, off = sections[m[3]]
        start = int(m[1], 16) - addr + off
        out[m[4]] = hashlib.sha256(image[start:start + int(m[2])]).hexdigest()
    return out


def resources(obj):
    with tempfile.TemporaryDirectory() as d:
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", unbundle(obj, d)], text=True)
    out = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        block = ".agpr_count:" + block
        get = lambda key: (re.search(r"\." + key + r":\s*(\S+)", block) or [None, "?"])[1]
        name = subprocess.check_output(["c++filt", get("name")], text=True).strip()
        out[name] = dict(vgpr=get("vgpr_count"), agpr=get("agpr_count"), sgpr=get("sgpr_count"),
                         vspill=get("vgpr_spill_count"), sspill=get("sgpr_spill_count"),
                         scratch=get("private_segment_fixed_size"), lds=get("group_segment_fixed_size"))
    return out


def _line(k, r):
    k = re.sub(r"^void pwg::", "", k)
    return (f"{r['vgpr']:>4} v {r['agpr']:>3} a {r['sgpr']:>3} s  spill {r['vspill']:>3}/{r['sspill']:>3}  "
            f"scratch {r['scratch']:>5}  lds {r['lds']:>6}  {k}")


def compare(other_dir, names):
    same = True
    for name in names:
        mine, theirs = os.path.join(BUILD, name + ".hip.o"), os.path.join(other_dir, name + ".hip.o")
        a, b = kernel_hashes(mine), kernel_hashes(theirs)
        only = sorted(set(a) ^ set(b))
        differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
        print(f"{name}: {len(a)} kernels here, {len(b)} there, {len(only)} in one only, {len(differ)} with other bytes")
        for k in only:
            print(f"  only {'here' if k in a else 'there'}: {k}")
        if differ:
            ra, rb = resources(mine), resources(theirs)
            for k in differ:
                dem = subprocess.check_output(["c++filt", k], text=True).strip()
                print("  here:  " + _line(dem, ra[dem]))
                print("  there: " + _line(dem, rb[dem]))
        same = same and not only and not differ
    return 0 if same else 1


BUILD = os.path.join(ROOT, "parallelwavegan_amd", "csrc", "build")


def main():
    if sys.argv[1:2] == ["--compare"]:
        sys.exit(compare(sys.argv[2], sys.argv[3:] or ["conv1d"]))
    for name in sys.argv[1:] or ["conv1d"]:
        obj = name if os.path.exists(name) else os.path.join(BUILD, name + ".hip.o")
        for k, r in sorted(resources(obj).items()):
            print(_line(k, r))


if __name__ == "__main__":
    main()
