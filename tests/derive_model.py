"""The model of derive_batch: three lines of Python, and the item rule's verdict beside them."""


def model(src, index=None, starts=None, ends=None, reverse=False, translate=None):
    """out[j] = X(src[i_j][a_j:b_j]); the items are taken as good (first_bad says whether they are)."""
    n_out = len(src) if index is None else len(index)
    cut = [src[j if index is None else int(index[j])][0 if starts is None else int(starts[j]):None if ends is None else int(ends[j])]
           for j in range(n_out)]
    cut = [c if translate is None else bytes(c).translate(translate) for c in cut]
    return [c[::-1] for c in cut] if reverse else cut


def first_bad(src, index=None, starts=None, ends=None):
    """-> (j, reason) of the smallest bad item (1: no such sequence, 2: start behind end, 3: end behind the sequence), or None."""
    n_out = len(src) if index is None else len(index)
    for j in range(n_out):
        i = j if index is None else int(index[j])
        if i >= len(src):
            return j, 1
        a = 0 if starts is None else int(starts[j])
        b = len(src[i]) if ends is None else int(ends[j])
        if a > b:
            return j, 2
        if b > len(src[i]):
            return j, 3
    return None


def offsets(seqs):
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    return offs
