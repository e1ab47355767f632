"""The --chores goldens (tests/golden/chores_*.chores / .segments, recorded by tests/golden/make_chores_golden.py) and
what the oracle says a chores run finds.

A chore is a target interval, a query interval and a strand (src/sequences.c read_chore: origin 1, closed; "* *" or
nothing for a whole sequence).  For each one lastz
  * sets hp->posFilter and the two intervals (origin 0, half open; the query's mirrored for the minus strand:
    src/lastz.c:1503-1512, 1627, resolve_chore_target / resolve_chore_query), so that filter_seed_hit_by_pos
    (src/seed_search.c:2269-2310) drops every seed hit whose window is not inside both; and
  * puts "fences" into BOTH sequences for the time of the search (start_one_strand, src/lastz.c:3028-3032,
    fence_sequence_interval, src/sequences.c:7789-7828): the bytes at s - 1 and at e become NUL, which ends every
    X-drop extension there.
The filter runs before the hit processor touches the diagonal hash, so a filtered hit leaves no trace, and the search is
that of a position table holding only the words inside the target interval, over the query interval, on the fenced
bytes.  The oracle says exactly that with the arguments it has: Table(start, end) and seed_hit_search(start, end)."""
import glob
import os

import numpy as np

from oracle import lzo
from lastz_amd import seqio
import helpers as H

NAMES = sorted(os.path.basename(p)[:-len(".chores")] for p in glob.glob(os.path.join(H.GOLDEN, "chores_*.chores")))


def sequences():
    (_, t), = seqio.read_fasta(os.path.join(H.GOLDEN, "pseudocat.fa"))
    return t, {name.strip(): q for name, q in seqio.read_fasta(os.path.join(H.GOLDEN, "pseudopig.fa"))}


def read_chores(name):
    """-> [(target interval or None, query name, query interval or None, strands)], intervals as the file has them"""
    out = []
    for line in open(os.path.join(H.GOLDEN, name + ".chores")):
        f = line.split("#")[0].split()
        if not f:
            continue
        assert f[0] == "cat"
        t_iv = None if f[1] == "*" else (int(f[1]), int(f[2]))
        rest = f[4:]
        q_iv = None
        if len(rest) >= 2:
            q_iv = None if rest[0] == "*" else (int(rest[0]), int(rest[1]))
            rest = rest[2:]
        strands = tuple(rest[0]) if rest else ("+", "-")
        out.append((t_iv, f[3], q_iv, strands))
    return out


def resolve(iv, n, minus=False):
    """resolve_chore_target / resolve_chore_query: origin 0, half open, the query's mirrored on the minus strand"""
    if iv is None:
        return 0, n
    s, e = iv[0] - 1, iv[1]
    return (n - e, n - s) if minus else (s, e)


def fenced(v, s, e):
    """fence_sequence_interval(seq, [s, e), 0): v[s - 1] and v[e] become NUL (v[len] is NUL already)"""
    w = v.copy()
    if s >= 1:
        w[s - 1] = 0
    if e < len(w):
        w[e] = 0
    return w


def searches(name):
    """per chore and strand of the file, in lastz's order: (query name, strand, fenced target, fenced query on that strand,
    target interval, query interval)"""
    t, qs = sequences()
    for t_iv, qname, q_iv, strands in read_chores(name):
        ts, te = resolve(t_iv, len(t))
        for strand in strands:
            q = qs[qname] if strand == "+" else seqio.revcomp(qs[qname])
            s2, e2 = resolve(q_iv, len(q), minus=(strand == "-"))
            yield qname, strand, fenced(t, ts, te), fenced(q, s2, e2), (ts, te), (s2, e2)


def oracle_hsps(tf, qf, t_iv, q_iv, masked, **kw):
    """the oracle's restricted search: the table of the words inside the target interval, searched over the query interval"""
    sd = lzo.seed()
    if t_iv[1] - t_iv[0] < sd.length or q_iv[1] - q_iv[0] < sd.length:
        return np.zeros(0, dtype=lzo.HSP_DTYPE), dict.fromkeys(("words", "raw_hits", "extensions", "bp_extended", "hsps"), 0)
    tab = lzo.Table(tf, sd, start=t_iv[0], end=t_iv[1])
    return lzo.seed_hit_search(tab, qf, masked, start=q_iv[0], end=q_iv[1], **kw)


def segments_text(rows):
    """--format=segments as lastz prints it: one header, then name1 start1 end1 name2 start2 end2 strand2 score
    (origin 1, closed; a minus-strand row counts along the reverse strand)"""
    return "#name1\tstart1\tend1\tname2\tstart2\tend2\tstrand2\tscore\n" + "".join(
        "cat\t%d\t%d\t%s\t%d\t%d\t%s\t%d\n" % (r[1], r[2], r[0], r[3], r[4], r[5], r[6]) for r in rows)


def oracle_segments(name):
    _, masked = H.scoring()
    rows = []
    for qname, strand, tf, qf, t_iv, q_iv in searches(name):
        hs, _ = oracle_hsps(tf, qf, t_iv, q_iv, masked)
        rows += H.hsps_as_tsv_rows(qname, strand, hs)
    return segments_text(rows)
