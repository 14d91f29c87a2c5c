"""Where a kernel waits for a global load before it issues the next independent one (CPU, reads assembly).

    hipcc <the Makefile's flags> -S --cuda-device-only -o net.s retargetvid_amd/csrc/svc_net.hip
    python tools/load_wait_census.py net.s [--only NAME_PART ...]

Per kernel, per basic block: the block's vector-memory loads and its `s_waitcnt vmcnt(N)` in order.  A wait is EXPOSED when it
drains the counter (vmcnt(0)) with exactly one load issued since the previous drain and another load follows it -- in the same
block, or in the next trip of a block that branches to itself: the two round trips are then paid one after the other.  Runs of
loads in front of a counted wait (vmcnt(N > 0)) are in flight together and are not listed.  Output: one line per kernel with
findings -- `loop` blocks (the trip count is the kernel's business) and `straight` blocks with the number of exposed waits."""
import re
import sys


def kernels(asm):
    entries = re.split(r'\n  - ', asm[asm.index('amdhsa.kernels:'):])
    for e in entries[1:]:
        m = re.search(r'\.name:\s+(\S+)', e)
        if not m:
            continue
        start = asm.find('\n%s:' % m.group(1))
        if start >= 0:
            yield m.group(1), asm[start:asm.index('s_endpgm', start)]


def exposed(body):
    out = []
    blocks = re.split(r'^(\.LBB\d+_\d+):', body, flags=re.M)
    for label, text in zip(['entry'] + blocks[1::2], [blocks[0]] + blocks[2::2]):
        ev = []
        for line in text.splitlines():
            t = line.strip()
            if re.match(r'(global|buffer)_load_', t):
                ev.append('L')
            else:
                w = re.match(r's_waitcnt.*vmcnt\((\d+)\)', t)
                if w:
                    ev.append('W0' if w.group(1) == '0' else 'W')
        loops = bool(re.search(r'^\s*s_cbranch_\w+\s+%s\s*$' % re.escape(label), text, re.M))
        n, since = 0, 0
        for i, e in enumerate(ev):
            if e == 'L':
                since += 1
            elif e == 'W0':
                more = 'L' in ev[i + 1:] or (loops and 'L' in ev)
                if since == 1 and more:
                    n += 1
                since = 0
        if n:
            out.append(('loop' if loops else 'straight', label, n))
    return out


def demangle(name):
    m = re.match(r'_Z\d+(k_\w+?)(I.*?E)?(v|P|[a-z]).*', name)
    return name if not m else m.group(1) + (m.group(2) or '')


def main(argv):
    only = argv[argv.index('--only') + 1:] if '--only' in argv else []
    asm = open(argv[1]).read()
    for name, body in kernels(asm):
        if only and not any(o in name for o in only):
            continue
        f = exposed(body)
        if f:
            print('%-60s %s' % (name[:60], '; '.join('%s %s x%d' % x for x in f)))


if __name__ == '__main__':
    main(sys.argv)
