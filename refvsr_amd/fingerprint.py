"""Host side of the parameter fingerprint (csrc/fingerprint.hip, refvsr_param_fingerprint): its numpy restatement, the chunk-table
builder and the policy that decides, per network call, how the packed weights are checked against the parameters.  Pure functions,
numpy only: everything here runs (and is tested) without a GPU.

  F = sum over all words of mix64((uint64(g) << 32) | word)   (mod 2^64)

word: the 32-bit pattern of an fp32 element; g: its index over the concatenated table, in table order, below 2^32; mix64:
splitmix64's finaliser, a bijection of the 64-bit words.  One changed word changes F, swapped contents change F, and the sum is
the same bits in every order."""
import numpy as np

MIX_MUL1 = 0xbf58476d1ce4e5b9          # splitmix64's finaliser: z ^= z >> 30; z *= MUL1; z ^= z >> 27; z *= MUL2; z ^= z >> 31
MIX_MUL2 = 0x94d049bb133111eb
CHUNK_WORDS = 4096                     # REFVSR_FINGERPRINT_CHUNK_WORDS
MAX_WORDS = 1 << 32                    # the global index is 32 bits wide
# one table entry as the kernel reads it: { const uint32_t* base; uint32_t g0; uint32_t n; }
CHUNK_DTYPE = np.dtype([('base', '<u8'), ('g0', '<u4'), ('n', '<u4')])

WEIGHT_CHECKS = ('auto', 'sync', 'off')


def mix64(z):
    """splitmix64's finaliser on a uint64 array (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over='ignore'):
        z ^= z >> np.uint64(30)
        z *= np.uint64(MIX_MUL1)
        z ^= z >> np.uint64(27)
        z *= np.uint64(MIX_MUL2)
        z ^= z >> np.uint64(31)
    return z


def words_of(a):
    """The 32-bit patterns of an array of 4-byte elements, in C order."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, 'the fingerprint is defined over 4-byte elements (got %s)' % a.dtype
    return a.reshape(-1).view(np.uint32)


def terms(words, g0=0):
    """The summands of F for `words` at global indices g0, g0 + 1, ..: a uint64 array."""
    words = np.asarray(words, dtype=np.uint32)
    if g0 + words.size > MAX_WORDS:
        raise ValueError('param_fingerprint: %d words do not fit the 32-bit global index' % (g0 + words.size))
    g = np.arange(g0, g0 + words.size, dtype=np.uint64)
    return mix64((g << np.uint64(32)) | words.astype(np.uint64))


def param_fingerprint_model(arrays):
    """F of a table of arrays of 4-byte elements (float32 parameters; any array whose bit patterns are meant), as a python int in
    [0, 2^64).  An empty table is refused."""
    arrays = list(arrays)
    if not arrays:
        raise ValueError('param_fingerprint: empty tensor list')
    total, g0 = np.uint64(0), 0
    with np.errstate(over='ignore'):
        for a in arrays:
            w = words_of(a)
            total = total + terms(w, g0).sum(dtype=np.uint64)
            g0 += w.size
    if g0 == 0:
        raise ValueError('param_fingerprint: the tensors hold no words')
    return int(total)


def as_int64(f):
    """F as the signed value a torch.int64 tensor shows for the same 64 bits."""
    f = int(f) & (2 ** 64 - 1)
    return f - 2 ** 64 if f >= 2 ** 63 else f


def chunk_table(word_counts, chunk_words=CHUNK_WORDS):
    """The chunks of a table of tensors with `word_counts` words each: a list of (tensor, first word inside the tensor, first global
    index, words), every chunk at most `chunk_words` words of one tensor, in table order -- every word in exactly one chunk, the
    global indices consecutive.  Tensors without words get no chunk.  An empty table (or one without words) and a table of 2^32
    words or more are refused."""
    counts = [int(n) for n in word_counts]
    if not counts or any(n < 0 for n in counts) or sum(counts) == 0:
        raise ValueError('param_fingerprint: empty tensor list')
    if sum(counts) >= MAX_WORDS:
        raise ValueError('param_fingerprint: %d words do not fit the 32-bit global index' % sum(counts))
    assert chunk_words >= 1
    out, g = [], 0
    for t, n in enumerate(counts):
        for off in range(0, n, chunk_words):
            m = min(chunk_words, n - off)
            out.append((t, off, g, m))
            g += m
    return out


def chunk_entries(pointers, word_counts, chunk_words=CHUNK_WORDS):
    """The chunk table as the kernel reads it: a CHUNK_DTYPE array, entry = (address of the chunk's first word, first global index,
    words); pointers: the tensors' data pointers (4-byte aligned)."""
    pointers = [int(p) for p in pointers]
    assert len(pointers) == len(word_counts)
    if any(p % 4 for p in pointers):
        raise ValueError('param_fingerprint: tensors must be 4-byte aligned')
    ch = chunk_table(word_counts, chunk_words)
    ent = np.zeros(len(ch), dtype=CHUNK_DTYPE)
    for i, (t, off, g, m) in enumerate(ch):
        ent[i] = (pointers[t] + 4 * off, g, m)
    return ent


def weight_check_policy(mode, has_frame_ids, first_frame, just_reset):
    """How one network call checks the packed weights against the parameters (config.weight_check): 'sync' | 'async' | 'none'.
      'off'  : never ('none': the host-side detector alone).
      'sync' : every call reads the fingerprint back before a kernel uses a weight.
      'auto' : 'sync' where a clip starts -- a first frame, the first call after construction / .to() / reset() / invalidate() --
               and 'async' everywhere else: the fingerprint is launched, read at the start of a later call.  Steady calls WITHOUT
               frame_ids are 'async' too: they wait for the window cache's content compare anyway, but one more device -> host
               read per call cost the plain call surface 3.3 % (profiles/weight_check_ab.txt: 182.7 -> 176.7 frames/s), past the
               1 % the check may cost -- has_frame_ids is part of the signature and decides nothing."""
    if mode not in WEIGHT_CHECKS:
        raise ValueError('weight_check must be one of %s, got %r' % (', '.join(WEIGHT_CHECKS), mode))
    if mode == 'off':
        return 'none'
    if mode == 'sync':
        return 'sync'
    if first_frame or just_reset:
        return 'sync'
    return 'async'
