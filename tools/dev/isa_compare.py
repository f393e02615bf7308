"""Development: compare the instruction text of every kernel in two gfx950 assembly files (`hipcc -S --cuda-device-only`
or the .s of `--save-temps`, with the build's flags) — before and after a change that must leave existing kernels alone.
Comments, directives, debug lines and labels are stripped and label references are numbered in order of appearance, so
that a renumbered basic block does not count as a change; per kernel: sha1 prefix and instruction-line count.
   python tools/dev/isa_compare.py before.s after.s [--alias 'REGEX=REPLACEMENT' ...]
--alias rewrites kernel names of `after` before matching (a template that gained a defaulted trailing parameter
mangles differently: `--alias 'ELb0EE=EE'` maps `kernel<..., false>` back onto `kernel<...>`)."""
import hashlib
import re
import sys


def kernels(path):
  """{kernel symbol: [normalised instruction lines]} for every .amdhsa_kernel of the file."""
  lines = open(path).read().splitlines()
  names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
  out, cur = {}, None
  for l in lines:
    m = re.match(r"^(\w+):", l)
    if m and m.group(1) in names:
      cur = m.group(1)
      out[cur] = []
      continue
    if cur is None:
      continue
    t = l.split(";")[0].strip()
    if t.startswith(".Lfunc_end") or t.startswith(".section") or t.startswith(".amdhsa_kernel"):
      cur = None
      continue
    if not t or t[0] == "." or t.endswith(":"):
      continue
    out[cur].append(t)
  for k, body in out.items():
    labels = {}
    def number(m):
      return labels.setdefault(m.group(0), "L%d" % len(labels))
    out[k] = [re.sub(r"\.LBB\d+_\d+", number, t) for t in body]
  return out


def main():
  args, aliases = [], []
  it = iter(sys.argv[1:])
  for a in it:
    if a == "--alias":
      pat, _, rep = next(it).partition("=")
      aliases.append((re.compile(pat), rep))
    else:
      args.append(a)
  before, after_raw = kernels(args[0]), kernels(args[1])
  after = {}
  for k, v in after_raw.items():
    name = k
    if k not in before:
      for pat, rep in aliases:
        if pat.sub(rep, k) in before:
          name = pat.sub(rep, k)
          break
    after[name] = v
  same = [k for k in before if k in after and before[k] == after[k]]
  changed = [k for k in before if k in after and before[k] != after[k]]
  print("kernels before %d, after %d; identical %d; changed %d; only before: %s" %
        (len(before), len(after), len(same), len(changed), sorted(set(before) - set(after))))
  for k in sorted(before):
    if k in after:
      print("%s %s %5d %s" % ("same" if k in same else "DIFF", hashlib.sha1("\n".join(after[k]).encode()).hexdigest()[:12],
                               len(after[k]), k))
  for k in sorted(set(after) - set(before)):
    print("new  %s %5d %s" % (hashlib.sha1("\n".join(after[k]).encode()).hexdigest()[:12], len(after[k]), k))
  return 1 if changed or set(before) - set(after) else 0


if __name__ == "__main__":
  sys.exit(main())
