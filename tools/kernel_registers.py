"""Registers, scratch and occupancy of every kernel of csrc/torbi_hip.hip, and which kernels fit beside the headline
forward instance.

Compiles the device code only (hipcc --cuda-device-only -Rpass-analysis=kernel-resource-usage, the flags of
torbi_amd._lib.build; no GPU needed) and reads the compiler's remarks.  A SIMD of gfx950 has 512 vector registers, handed
out in steps of 8 per wave.  The headline instance keeps `--waves` (4) of its waves on every SIMD -- one workgroup of sixteen
per compute unit, which its LDS tile allows -- so a kernel of another stream gets a wave in only if its own allocation fits
what those leave, and it has to do without scratch to stay there at any speed.

    python tools/kernel_registers.py [--only REGEX] [--headline REGEX] [--waves 4] > profiles/<name>_kernel_registers.txt
"""
import argparse
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILE_REGISTERS = 512        # vector registers of a SIMD (gfx950: unified VGPR + AGPR file, per lane)
GRANULE = 8                 # allocation step per wave
HEADLINE = r'resident_forward_kernel<16, 6, true, 1, false, 16, false>'

FIELDS = {
    'VGPRs': 'vgprs', 'AGPRs': 'agprs', 'TotalSGPRs': 'sgprs', 'SGPRs': 'sgprs', 'ScratchSize [bytes/lane]': 'scratch',
    'Occupancy [waves/SIMD]': 'occupancy', 'LDS Size [bytes/block]': 'lds',
}


def allocated(kernel):
    return (kernel['vgprs'] + kernel.get('agprs', 0) + GRANULE - 1) // GRANULE * GRANULE


def compile_remarks():
    from torbi_amd import _lib
    cmd = [_lib.hipcc(), '--offload-arch=gfx950', '--cuda-device-only', '-c', '-O3', '-std=c++17', '-ffp-contract=off',
           '-fno-slp-vectorize', '-Wno-pass-failed', f'-I{_lib.INCLUDE}', '-Rpass-analysis=kernel-resource-usage',
           '-o', os.devnull, _lib.SOURCE]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr)
        raise SystemExit(f'device compile failed ({done.returncode})')
    return done.stderr


def demangle(names):
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    for cand in ('/opt/rocm/llvm/bin/llvm-cxxfilt', '/opt/rocm/lib/llvm/bin/llvm-cxxfilt'):
        if not tool and os.path.exists(cand):
            tool = cand
    if not tool or not names:
        return list(names)
    out = subprocess.run([tool], input='\n'.join(names) + '\n', stdout=subprocess.PIPE, text=True, check=True).stdout
    return out.splitlines()


def parse(remarks):
    """[{name, vgprs, agprs, sgprs, scratch, occupancy, lds}] in the order of the remarks."""
    kernels, cur = [], None
    for line in remarks.splitlines():
        m = re.search(r'remark:\s+(Function Name|[A-Za-z]+(?: Size)?(?: \[[^\]]+\])?): (\S+)(?: \[-Rpass-analysis[^\]]*\])?\s*$', line)
        if not m:
            continue
        key, value = m.group(1), m.group(2)
        if key == 'Function Name':
            cur = {'name': value}
            kernels.append(cur)
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = int(value)
    kernels = [k for k in kernels if 'vgprs' in k]
    for k, name in zip(kernels, demangle([k['name'] for k in kernels])):
        k['name'] = re.sub(r'^void ', '', name)
        k['name'] = re.sub(r'\((?:[^()]|\([^()]*\))*\)$', '', k['name'])      # drop the parameter list
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--only', default=None, help='print only the kernels whose name matches this regular expression')
    ap.add_argument('--headline', default=re.escape(HEADLINE), help='the forward instance the others have to fit beside')
    ap.add_argument('--waves', type=int, default=4, help='waves per SIMD the headline instance keeps resident')
    ap.add_argument('--remarks', default=None, help='read the compiler remarks from this file instead of compiling')
    args = ap.parse_args()
    remarks = open(args.remarks).read() if args.remarks else compile_remarks()
    kernels = parse(remarks)
    head = [k for k in kernels if re.search(args.headline, k['name'])]
    if len(head) != 1:
        raise SystemExit(f'{len(head)} kernels match the headline pattern {args.headline!r}')
    free = FILE_REGISTERS - args.waves * allocated(head[0])
    print(f'headline: {head[0]["name"]}')
    print(f'  {head[0]["vgprs"]} VGPRs + {head[0].get("agprs", 0)} AGPRs -> {allocated(head[0])} allocated per wave, '
          f'{args.waves} waves per SIMD resident: {free} of {FILE_REGISTERS} registers free, LDS {head[0].get("lds", 0)} B static')
    print(f'{"VGPRs":>6} {"alloc":>6} {"scratch":>8} {"occ":>4} {"LDS":>7}  fits  kernel')
    for k in sorted(kernels, key=lambda k: k['name']):
        if args.only and not re.search(args.only, k['name']):
            continue
        fits = allocated(k) <= free and k.get('scratch', 0) == 0
        print(f'{k["vgprs"] + k.get("agprs", 0):>6} {allocated(k):>6} {k.get("scratch", 0):>8} {k.get("occupancy", 0):>4} '
              f'{k.get("lds", 0):>7}  {"yes " if fits else "no  "}  {k["name"]}')


if __name__ == '__main__':
    main()
