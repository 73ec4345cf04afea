"""Static instruction counts and resource usage per kernel: one table row per kernel.

usage: python tools/isa_counts.py file.s remarks.txt [kernel-substring ...]

file.s: the device listing (hipcc -S --cuda-device-only); remarks.txt: the stderr of the same compile
with -Rpass-analysis=kernel-resource-usage.  Counts VALU instructions (v_*), v_readlane, v_writelane,
s_nop and scratch ops between the kernel's label and its end, and takes the spill counts, scratch size
and occupancy from the remarks.
"""
import re
import sys

s = open(sys.argv[1]).read()
rem = open(sys.argv[2]).read()
pats = sys.argv[3:] or [""]

usage = {}
cur = None
for line in rem.splitlines():
  m = re.search(r"remark: (?:.*?)Function Name: (\S+)", line)
  if m:
    cur = usage.setdefault(m.group(1), {})
    continue
  m = re.search(r"remark:\s+(?:.*?)([A-Za-z][A-Za-z ]*?)(?: \[bytes/lane\]| \[waves/SIMD\]| \[bytes/block\])?: (\d+)", line)
  if m and cur is not None:
    cur[m.group(1).strip()] = int(m.group(2))

print("| kernel | static VALU | v_readlane | v_writelane | s_nop | scratch ops | SGPR spills | VGPR spills | scratch B/lane | VGPRs | waves/SIMD |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
for m in re.finditer(r"^(_Z\S+):\s*;", s, re.M):
  name = m.group(1)
  if not any(p in name for p in pats):
    continue
  body = s[m.start():s.index(".Lfunc_end", m.end())].split("\n")
  ops = [l.split()[0] for l in body if l.startswith("\t") and l.split() and not l.split()[0].startswith((".", ";"))]
  n = lambda pre: sum(1 for o in ops if o.startswith(pre))
  u = usage.get(name, {})
  print(f"| `{name}` | {n('v_')} | {n('v_readlane')} | {n('v_writelane')} | {n('s_nop')} | {n('scratch_')} | "
        f"{u.get('SGPRs Spill', '?')} | {u.get('VGPRs Spill', '?')} | {u.get('ScratchSize', '?')} | {u.get('VGPRs', '?')} | {u.get('Occupancy', '?')} |")
