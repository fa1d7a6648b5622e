"""Python statement of the drafter's three rules (csrc/kh_lookup.h, kh_lookup_draft): the twin the tests compare with."""


def draft(seq, hint, ngram_max, ngram_min, cap):
    seq, hint = list(seq), list(hint or [])
    for g in range(min(ngram_max, len(seq)), ngram_min - 1, -1):
        key = seq[len(seq) - g:]
        # 1. the EARLIEST place in the hint with a follower; 2. else the MOST RECENT earlier place in the sequence
        js = [j for j in range(len(hint) - g) if hint[j:j + g] == key]
        if js:
            return hint[js[0] + g:][:cap]
        js = [j for j in range(len(seq) - g) if seq[j:j + g] == key]
        if js:
            return seq[js[-1] + g:][:cap]
    return []
