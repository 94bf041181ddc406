"""A strict validator of one LZ4 block: every rule the format puts on a block that a compressor writes, checked on the bytes
alone.  The reference's safe decoder accepts blocks that break the end rules (a match that starts within the last 12 bytes,
fewer than 5 last literals), so "the decoder gives the input back" does not show that an encoder kept them; other LZ4
decoders reject or mis-decode such blocks.  tests/test_encode_cases.py pins the validator (the oracle's and the
reference's own blocks pass; hand-built violations fail by the right rule), tests/test_encode_edges_gpu.py holds every GPU
encoder to it.

Test infrastructure only.
"""

MINMATCH = 4
LASTLITERALS = 5      # the last 5 bytes of a block are literals
MFLIMIT = 12          # a match starts at least 12 bytes before the block's end
MIN_LENGTH = MFLIMIT + 1

# the rules, by the name a BlockRuleError carries
BOUNDS = "bounds"                  # a token, length byte, literal or offset lies outside the block
END = "end"                        # the walk does not end at len(block) with exactly n bytes of output
LAST_SEQUENCE = "last sequence"    # the last sequence's token has a non-zero low nibble
OFFSET = "offset"                  # an offset of 0, or one that reaches in front of the output (and the dictionary)
SHORT = "short block"              # a match in a block of fewer than 13 bytes
MATCH_START = "last 12 bytes"      # a match starts within the last 12 bytes
LAST_LITERALS = "last 5 bytes"     # a match reaches into the last 5 bytes
BOUND = "compressBound"            # the block is larger than LZ4_compressBound(n)


class BlockRuleError(AssertionError):
    """A block breaks a rule: .rule is one of the names above, the message names the rule and the position."""

    def __init__(self, rule, message):
        AssertionError.__init__(self, "%s: %s" % (rule, message))
        self.rule = rule


def compress_bound(n):
    return n + n // 255 + 16


def check_block(block, n, dict_len=0):
    """Walks one block that must decode to n bytes, with dict_len bytes of dictionary in front of its output.  Raises
    BlockRuleError (an AssertionError) naming the rule and the position; returns (sequences with a match, largest offset,
    output position of the last match's start or -1, matches that reach into the dictionary)."""
    block = bytes(block)
    size = len(block)
    if size > compress_bound(n):
        raise BlockRuleError(BOUND, "%d bytes for %d, LZ4_compressBound is %d" % (size, n, compress_bound(n)))
    i = pos = 0
    seqs = max_off = into_dict = 0
    last_start = -1

    def length(i, v, what, at):
        if v == 15:
            while True:
                if i >= size:
                    raise BlockRuleError(BOUNDS, "%s length of the sequence at byte %d runs past the block" % (what, at))
                b = block[i]
                i += 1
                v += b
                if b != 255:
                    break
        return i, v

    while True:
        if i >= size:
            raise BlockRuleError(BOUNDS, "a token at byte %d, the block has %d (output position %d of %d)" % (i, size, pos, n))
        at = i
        tok = block[i]
        i, lit = length(i + 1, tok >> 4, "literal", at)
        if i + lit > size:
            raise BlockRuleError(BOUNDS, "%d literals at byte %d, the block has %d" % (lit, i, size))
        i += lit
        pos += lit
        if pos > n:
            raise BlockRuleError(END, "literals up to output position %d of %d (sequence at byte %d)" % (pos, n, at))
        if pos == n:
            # nothing can follow: a match needs 4 more bytes of output.  This is the last sequence.
            if i != size:
                raise BlockRuleError(END, "the output is complete at byte %d, the block has %d" % (i, size))
            if tok & 15:
                raise BlockRuleError(LAST_SEQUENCE, "the last token (byte %d) has the low nibble %d" % (at, tok & 15))
            return seqs, max_off, last_start, into_dict
        if i == size:
            raise BlockRuleError(END, "the block ends at output position %d of %d" % (pos, n))
        if i + 2 > size:
            raise BlockRuleError(BOUNDS, "an offset at byte %d, the block has %d" % (i, size))
        off = block[i] | (block[i + 1] << 8)
        i, ml = length(i + 2, tok & 15, "match", at)
        ml += MINMATCH
        if not 1 <= off <= 65535 or off > pos + dict_len:
            raise BlockRuleError(OFFSET, "offset %d at output position %d with %d bytes of dictionary (sequence at byte %d)"
                                 % (off, pos, dict_len, at))
        if n < MIN_LENGTH:
            raise BlockRuleError(SHORT, "a match at output position %d of a block of %d bytes" % (pos, n))
        if pos > n - MFLIMIT:
            raise BlockRuleError(MATCH_START, "a match starts at output position %d of %d (sequence at byte %d)" % (pos, n, at))
        if pos + ml > n - LASTLITERALS:
            raise BlockRuleError(LAST_LITERALS, "a match of %d bytes at output position %d of %d: the last 5 bytes are not "
                                 "literals (sequence at byte %d)" % (ml, pos, n, at))
        seqs += 1
        max_off = max(max_off, off)
        last_start = pos
        into_dict += off > pos
        pos += ml
