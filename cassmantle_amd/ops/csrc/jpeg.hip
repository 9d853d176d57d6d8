// Batched baseline JPEG (JFIF) encoder for gfx950: uint8 [B][H][W][3] images in HBM -> one
// complete JPEG byte string per image in one payload buffer.  ops/jpeg_format.py is the pure
// numpy reference of the same contract and owns the tables (quantisation, Huffman, header bytes),
// which arrive here as small device arrays.
//
// THE BYTE CONTRACT (integer arithmetic end to end; `>>` is an arithmetic shift = floor division)
//
//   Geometry.  Sampling "420": MCU = 16x16 pixels = blocks Y00 Y01 Y10 Y11 Cb Cr (6); "444":
//   MCU = 8x8 pixels = blocks Y Cb Cr (3).  MCUs in raster order; pixel (y, x) outside the image
//   reads (min(y, H-1), min(x, W-1)).
//
//   Colour (16-bit fixed point, JFIF / BT.601 full range), per pixel:
//     Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//     Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//     Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
//   Chroma 2x2 mean (420):  c = (c00 + c01 + c10 + c11 + 2) >> 2, after the conversion.
//   Level shift: s = sample - 128.
//
//   DCT, separable, matrix C[k][n] = round(2^13 * c(k)/2 * cos((2n+1) k pi / 16)) (DCTM below;
//   its 8 distinct magnitudes are 2896 4017 3784 3406 2896 2276 1567 799):
//     rows:     t[r][k] = (sum_n C[k][n] * s[r][n] + 2^8)  >> 9     (4 fraction bits kept)
//     columns:  f[k][c] = (sum_n C[k][n] * t[n][c] + 2^13) >> 14    (8 x the DCT coefficient)
//   Quantisation by Q (natural order, luma table for Y blocks, chroma for Cb / Cr), round half
//   away from zero:  v = sign(f) * ((|f| + 4 Q) / (8 Q));  AC values are clamped to +-1023 (the
//   baseline Huffman tables have no AC category 11).  Coefficients are stored in zig-zag order.
//
//   Entropy coding.  A restart interval is `restart` consecutive MCUs (the last may be short):
//   DC predictors of the three components start at 0, blocks are coded with the standard
//   category / run-length symbols (ZRL for runs of 16 zeros, EOB when the block ends in zeros),
//   code word and value bits MSB first, every 0xFF byte followed by a stuffed 0x00, the last
//   byte padded with 1-bits.  Interval i of an image is followed by RST(i & 7), the last one by
//   EOI.  Intervals are therefore independent, byte-aligned units of work.
//
// Kernels: transform (one wave per MCU) -> count (one lane per interval runs the coder without
// storing) -> exclusive scan per image and over the batch -> write (the same coder, storing at
// the final offsets) + header copy.  Device memory beyond coefficients and payload is two
// 32-bit words per interval.
//
// THE DECODE CONTRACT (jpeg_format.reconstruct is its numpy reference): the pixels a libjpeg
// decoder with its defaults (ISLOW inverse DCT, fancy upsampling; PIL) returns for the bytes
// above.  They are a function of the quantised coefficients and Q alone, so they are computed
// from the coefficient buffer the transform filled; nothing is entropy-decoded.  Integer
// arithmetic, 32-bit words (the dequantised values come from the DCT above of 8-bit samples;
// the reference asserts the width), `>>` arithmetic.
//
//   Dequantise.  d = coefficient * Q at its natural position (luma table for Y, chroma for Cb / Cr).
//
//   Inverse DCT (jidctint, CONST_BITS 13, PASS1_BITS 2): the 8 columns first, then the 8 rows.
//   One 8-point pass on i0..i7:
//     even:  z1 = (i2 + i6) * 4433;  t2 = z1 - i6 * 15137;  t3 = z1 + i2 * 6270
//            t0 = (i0 + i4) << 13;   t1 = (i0 - i4) << 13
//            t10 = t0 + t3;  t13 = t0 - t3;  t11 = t1 + t2;  t12 = t1 - t2
//     odd:   a = i7, b = i5, c = i3, d = i1
//            z1 = a + d;  z2 = b + c;  z3 = a + c;  z4 = b + d;  z5 = (z3 + z4) * 9633
//            a *= 2446;  b *= 16819;  c *= 25172;  d *= 12299
//            z1 *= -7373;  z2 *= -20995;  z3 = z3 * -16069 + z5;  z4 = z4 * -3196 + z5
//            a += z1 + z3;  b += z2 + z4;  c += z2 + z3;  d += z1 + z4
//     out 0..7 = t10+d  t11+c  t12+b  t13+a  t13-a  t12-b  t11-c  t10-d, each (v + 2^(s-1)) >> s
//     with s = 11 in the column pass and s = 18 in the row pass.
//   Sample = clamp(result + 128, 0, 255).
//
//   Chroma (420; 444 has none).  Only the ch = ceil(H/2) x cw = ceil(W/2) real samples of a
//   chroma plane are read, indices clamped to them.  Output row 2r takes neighbour row r-1, row
//   2r+1 takes r+1:  s[x] = 3 c[r][x] + c[neighbour][x];  then
//     out[2x] = (3 s[x] + s[x-1] + 8) >> 4        out[2x+1] = (3 s[x] + s[x+1] + 7) >> 4
//   With cw <= 2 libjpeg replicates instead: out[y][x] = c[y >> 1][x >> 1].
//
//   Colour, cb = Cb - 128, cr = Cr - 128, each clamped to 0..255:
//     R = Y + ((91881 cr + 32768) >> 16)
//     G = Y + ((-22554 cb - 46802 cr + 32768) >> 16)
//     B = Y + ((116130 cb + 32768) >> 16)
//   The output is the H x W crop.
//
// Kernels: idct (one wave per MCU, the mirror of transform; uint8 samples into padded planes) ->
// colour (upsampling crosses block and MCU borders, so it reads the planes: 4 pixels per lane).
//
// THE ENTROPY DECODE CONTRACT (jpeg_format.entropy_decode is its numpy reference, jpeg_entropy_dec.h
// the routine): the bytes of one restart interval of any baseline scan in scope (SOF0, 8-bit,
// 4:2:0 or 4:4:4, one interleaved scan, the stream's own DQT / DHT; jpeg_format.parse) -> the
// quantised zig-zag coefficients the DECODE CONTRACT starts from.  The host finds the intervals
// (in entropy-coded data every 0xFF is followed by 0x00 or by a marker), so an interval is the
// bytes between two markers, markers excluded.
//
//   Bit order.  Bytes in stream order, bits of a byte MSB first; a code word and the value bits
//   after it are read in that order.
//   Unstuffing.  0xFF 0x00 is the data byte 0xFF.  A 0xFF followed by anything else, or ending the
//   interval, ends the data there.  Bits left after the last block (the padding) are ignored.
//   Canonical codes (T.81 Annex C).  For a DHT (BITS[1..16], HUFFVAL): code = 0; for l = 1..16 the
//   next BITS[l] values get the codes code, code + 1, ... of length l; then code <<= 1.  The
//   symbol is that of the shortest l whose first l bits are such a code.
//   EXTEND.  A symbol's size s is followed by s bits u (MSB first): v = u if u >= 2^(s-1), else
//   v = u - 2^s + 1.  s = 0 has no bits and v = 0.
//   Block.  DC symbol = s (<= 11): coefficient 0 = predictor + v, which becomes the predictor of
//   its component.  Then from k = 1, AC symbol (run << 4) | s: 0x00 (EOB) ends the block, the
//   rest is zero; 0xF0 (ZRL) is k += 16; otherwise (1 <= s <= 10) k += run, coefficient k = v,
//   k += 1.  The block also ends after k = 63.  Luma blocks use the tables the first component
//   names, chroma blocks the other two components' (shared) tables.
//   DC prediction.  The three predictors start at 0 in every interval.  Interval i holds the MCUs
//   i * restart .. min((i + 1) * restart, mcus) - 1 in raster order (no DRI: all of them).
//   Errors, the first in decode order being the interval's status:
//     TRUNCATED (1)  a code word or value bits are wanted beyond the end of the data
//     BAD_CODE  (2)  16 bits that start no code word; a DC size above 11; an AC size above 10; an
//                    AC symbol with s = 0 other than EOB and ZRL
//     OVERRUN   (3)  k beyond 63 after a run, or after a ZRL (no coefficient can follow it)
//     WIDE      (4)  the refusal rule: with d = coefficient * Q, a block with any |d| > T or
//                    sum d^2 > T^2, T = 2047 (jpeg_format.WIDE_T: the 32-bit words of the idct
//                    kernel and the 16-bit words of libjpeg's SIMD inverse DCT hold everything
//                    below it, and no block of 8-bit samples reaches it)
//   An interval with an error is abandoned; the status of a call is the error of its lowest
//   interval (image * intervals + interval), and then no pixels are returned: a refusal, never
//   different pixels.
//
// Kernel: entropy decode, one lane per restart interval like the coder it mirrors, the decode
// tables (about 4 KiB) in LDS; the coefficient buffer is zeroed first and only non-zero
// coefficients are stored.
//
// THE CHUNKED ENTROPY DECODE CONTRACT (jpeg_format.entropy_decode_chunked is its numpy model,
// jpeg_entropy_sync.h the lane run): the same coefficients and the same refusals as the ENTROPY
// DECODE CONTRACT, with one lane per fixed-size byte chunk of an interval instead of one per
// interval.  A Huffman decoder started at a wrong position falls into step with the true decode
// after a short stretch, so lanes start on guesses and iterate until every lane's start equals
// its predecessor's exit.
//
//   Chunks.  The raw bytes of every interval (stuffed zeros included) are cut into chunks of cb
//   bytes, the last one shorter; chunks never cross an interval.  cb = the smallest multiple of
//   16 that is >= chunk_bytes (itself >= 16) and leaves the longest interval of the call at most
//   1024 chunks.  An interval is shorter than 2^28 bytes (bit positions are 32-bit words).  A
//   symbol is at most 27 bits = 5 data bytes = 10 raw bytes, so an exit lies less than 16 bytes
//   past the chunk end: inside the next chunk's cb, and a 7-bit offset from the chunk end.
//   State (p, blk, k).  p = raw bit position in the interval of the next symbol's first bit,
//   never inside a stuffed 0x00; blk = the block of the MCU it belongs to (selects luma / chroma
//   tables as in jpeg_decode_interval); k = 0: a DC symbol is next, else the zig-zag index of the
//   AC symbol.  A symbol is a code word plus its value bits; a ZRL is a symbol.
//   Lane run.  From its start a lane decodes symbols while p is before its chunk's end, with the
//   structural rules above (TRUNCATED, BAD_CODE, OVERRUN; a 0xFF not followed by 0x00 ends the
//   data), no predictor and no WIDE rule.  It counts the DC symbols it decoded (blocks started)
//   and exits in the state at the first symbol boundary at or past the chunk end, or in "error"
//   (the last lane of an interval runs to the interval's end and normally ends in TRUNCATED
//   inside the padding).  What a lane makes of bytes behind the end of the data is left open
//   (the kernel decodes them like any others, the numpy model stops with TRUNCATED): no valid
//   chain reaches them, because a symbol that needs bits from there is TRUNCATED.
//   Rounds (Jacobi).  Round 0: lane 0 of an interval starts at (0, 0, 0), lane c > 0 at (first
//   bit of its chunk, 0, 0), one byte later when the chunk's first byte is a stuffed zero (the
//   byte before it in the interval is 0xFF).  Round r + 1: a lane whose predecessor's round-r
//   exit is a state other than its own start adopts it and runs again; every other lane rests.
//   The iteration ends with the first round in which no lane runs; `rounds` counts the rounds in
//   which one did (the largest count of any interval of the call).  Lane c is final after round
//   c, so rounds <= chunks of the longest interval, and the loop is bounded by that.
//   Valid chain.  Lane 0 is valid; lane c is valid if lane c - 1 is valid and exited in a state
//   (after convergence lane c's start).  The valid lanes' runs, in order, are the serial decode.
//   Placement.  The exclusive scan of the valid lanes' block counts over the interval is the
//   index of the first block a lane starts (a lane that starts inside a block, k != 0, continues
//   the block before it).  Blocks at or past the interval's block count are dropped, and so are
//   errors in them: the serial decoder never looks past its last block.
//   Write pass.  Valid lanes run once more and store into the zeroed buffer: the DC difference at
//   coefficient 0, non-zero AC values at their k; every store index is checked.  They count the
//   blocks inside the image they completed.
//   DC pass.  Per interval and component an inclusive 32-bit prefix sum of the DC differences in
//   block order replaces them.  A predictor with |predictor * Q| > T is not stored (never
//   truncated to 16 bits) and raises the flag.  The first such predictor in block order is below
//   T + 2^11 in magnitude, so a wrapped sum cannot hide it.
//   Check pass.  One thread per block: |coefficient * Q| <= T for all 64 and sum d^2 <= T^2.
//   Flag.  Raised by a structural error of a valid lane in a block inside the image, by the DC
//   and check passes, by an interval outside the staged bytes; and the call counts as flagged
//   when the valid lanes completed fewer blocks than the image has.
//   Refusals are the serial decoder's.  A flagged call zeroes the buffer and runs
//   jpeg_entropy_decode_kernel on the same staged bytes; its status decides what is raised (and
//   were it OK, its coefficients would be used).  The chunked path guarantees: serial OK => no
//   flag and equal coefficients; serial error => flag.
//
// Kernels: sync (one workgroup of up to 1024 lanes per group of consecutive intervals of one
// image holding at most 1024 chunks; decode tables, packed exits and the scans in LDS; rounds
// separated by block-uniform barriers; validity and block scans, then the write pass) -> DC
// prefix (one workgroup per interval) -> check (one thread per block).  The host cuts the groups
// and stages them with the bytes.
//
// BLOCK-PARALLEL ENTROPY CODER (jpeg_format.entropy_blocks is its numpy model, jpeg_entropy_blk.h
// the per-block coder and the stuffing piece): the bytes of the BYTE CONTRACT for any restart
// interval, none included (no DRI: the image is one interval), with one lane per 8x8 block instead
// of one per interval.  A block's code bits depend on its 64 coefficients and on the DC value of
// the previous block of its component only, and both are in the coefficient buffer.
//
//   DC predictor.  Of block k of MCU m: Y blocks of an MCU follow each other (k > 0: block k - 1
//   of the MCU), the first follows the last Y block of MCU m - 1; Cb / Cr follow Cb / Cr of MCU
//   m - 1.  In the first MCU of an interval those are 0.
//   Bits.  A lane runs the coder of the byte contract on its block without storing: its bit length
//   (4 .. 1660; the bound is longest DC code + 11 + 63 * (longest AC code + 10)).
//   Scan.  The exclusive scan of the lengths over the interval is every block's bit offset in the
//   interval's unstuffed string; the sum is the string's bit count, ceil(bits / 8) its bytes.
//   Pack.  A lane runs the same coder again and puts its bits, MSB first, at its offset into the
//   string's 32-bit words; the lane of the interval's last block appends the 1-bits that pad the
//   last byte.  A word that lies inside one block has one writer, which stores it.  Up to 7 blocks
//   start in one word (a flat chroma block is 4 bits), so the first and the last word of a block
//   are merged with atomicOr; exactly those words (the word every block starts in, and the word
//   the interval ends in) were zeroed by the scan pass, one store per block, nothing else is.
//   Stuff.  The string is cut into pieces of 32 bytes (the last one shorter); a lane counts its
//   piece's 0xFF bytes, the scan of piece length + count over the interval is the piece's place
//   in the interval's bytes, and the total + 2 (RSTn / EOI) is the interval's length, from which
//   jpeg_scan_image_kernel and jpeg_scan_batch_kernel give the image offsets as before.  After
//   the host has read those, the lanes count again, scan, and copy their pieces to their final
//   place, a 0x00 behind every 0xFF; the interval's first lane writes the marker.
//   Bounds.  The string of an interval has a slot of ceil(blocks * 1660 / 32) words.  Every word
//   index is checked against the slot, every payload index against the payload's size; a refused
//   index raises an error word (count passes: behind the image offsets, read with them) or byte
//   (write pass: behind the payload, read with it) and stores nothing.
//
// Kernels: transform -> bits (one lane per block) -> scan (one workgroup per interval, tiles of
// up to 1024 blocks with a running sum) -> pack (one lane per block) -> stuff<count> (one
// workgroup per interval, tiles of up to 1024 pieces) -> the two scans of the interval coder ->
// stuff<write> + header copy.  Every dependency is a kernel boundary or a barrier inside one
// workgroup, every loop is bounded by a size known at launch.  Device memory beyond coefficients
// and payload: one word per block, one per interval, and the slots (208 bytes per block, of which
// 4 bytes per block + 4 per interval are zeroed).
//
// OPTIMISED HUFFMAN TABLES (jpeg_format.symbol_counts / optimal_table are the numpy model,
// jpeg_huff_opt.h the builder): with huffman = "optimized" every image of the batch is coded with,
// and carries in its DHT, the four tables libjpeg's jpeg_gen_optimal_table (T.81 K.2) builds for
// the image's own coefficients.  The coefficients, and so the decoded pixels, do not change.
//
//   Counts.  freq[t][s], t = DC luma, DC chroma, AC luma, AC chroma: how often the entropy coder
//   of the byte contract emits symbol s of table t for the image: the category of every DC
//   difference (against the DC predictor of the block coder, restart intervals included), every
//   (run << 4) | size, ZRL and EOB.  32-bit words: an image has fewer than 2^31 coefficients
//   (blocks * 64 < 2^31), larger ones are refused.
//   Table from freq[0 .. 255]:
//     1. freq[256] = 1, the reserved symbol: no code is all ones.
//     2. codesize[0 .. 256] = 0, others[0 .. 256] = -1.
//     3. Repeat: c1 = the index with the smallest non-zero freq, the largest index among equal
//        values; c2 = the same search with c1 left out; if there is none, stop.
//        freq[c1] += freq[c2]; freq[c2] = 0; codesize of c1 and of every index on its others chain
//        + 1; the chain's end is linked to c2; codesize of c2 and of its chain + 1.
//     4. bits[l] = the number of indices with codesize l, l up to 32 (a longer code is refused, as
//        libjpeg refuses it; 2^31 symbols can reach it only with Fibonacci-like counts).
//     5. For i = 32 .. 17, while bits[i] > 0: j = i - 2; while bits[j] == 0, j -= 1;
//        bits[i] -= 2; bits[i - 1] += 1; bits[j + 1] += 2; bits[j] -= 1.
//     6. From i = 16 down to the first bits[i] > 0: bits[i] -= 1 (the reserved symbol leaves).
//     7. vals = for l = 1 .. 32, for j = 0 .. 255 ascending: j if codesize[j] == l.
//   Codes are canonical from (bits[1 .. 16], vals) as in the ENTROPY DECODE CONTRACT.  A table
//   lists only the symbols that occur (a table without any is 17 bytes of DHT).
//   Header.  The segments and their order are the byte contract's, with one DHT segment holding
//   the image's tables in the order DC luma, AC luma, DC chroma, AC chroma; its length, and so the
//   header's, differs per image.
//   Bounds.  Any code, a DC one included, can be 16 bits long: a block codes to at most
//   16 + 11 + 63 * 26 = 1665 bits, and the block coder's slots are sized with that.
//
// Kernels, between transform and the coders' count pass: histogram (one lane per block in the
// geometry of the bits kernel, the coder's own symbol walk with a counting sink, a HUFF_WORDS
// histogram in LDS per workgroup flushed with integer atomicAdd into freq[B][HUFF_WORDS], zeroed
// before) -> build (one workgroup per image, one wave per table; freq, codesize, others, bits in
// LDS; the two searches of step 3 are wave reductions on the 64-bit key (freq, reversed index);
// after a barrier the workgroup writes the image's (length << 16) | code words, its header =
// the constant bytes before the DHT + its DHT + the constant bytes behind, and hdr_len[b]; a
// refused table gives hdr_len[b] = 0, which the host reads with the image offsets).  Both coders
// then read the image's words and hdr_len[b].  The interval kernel's 64 lanes and the block
// kernels' BLK_LANES would straddle two images, so in this mode their grids get an image dimension
// (blockIdx.y = image, blockIdx.x tiles the image's intervals / blocks): a workgroup holds one
// image's table in LDS as before.  One launch per pass still, and at most 65535 images per call.
// The host flow is unchanged: no copy or synchronisation is added.
//
// LIBJPEG FORWARD CONTRACT (transform = "libjpeg"; jpeg_format.coefficients_libjpeg is its numpy
// model, jpeg_fdct_lj.h the arithmetic): the coefficients, and with the header layout below and no
// restart markers the whole file, that libjpeg (PIL's Image.save(format="JPEG", quality=q)) writes
// for the same pixels.  It replaces the geometry's edge rule, the chroma mean and the DCT of the
// byte contract; colour, level shift, quantisation formula, zig-zag order and entropy coding are
// the byte contract's.  Integer arithmetic in 32-bit words (the model asserts the width).
//
//   Edges, 4:4:4.  Every plane is replicated (last column, last row) up to whole 8x8 blocks.
//   Edges and chroma, 4:2:0.  ch = ceil(H/2), cw = ceil(W/2); the chroma plane has cbh = ceil(ch/8)
//   x cbw = ceil(cw/8) blocks (= the MCU grid).  Full-resolution Cb / Cr are replicated to 2 ch
//   rows (an even row count, no further) and to 16 cbw columns; then
//     c[r][x] = (p[2r][2x] + p[2r][2x+1] + p[2r+1][2x] + p[2r+1][2x+1] + bias) >> 2,
//     bias = 1 for even x, 2 for odd x;
//   then the downsampled rows are replicated from ch to 8 cbh.  In source coordinates: chroma
//   sample (r, x) reads rows y0 = 2 min(r, ch-1) and min(y0+1, H-1), columns min(2x, W-1) and
//   min(2x+1, W-1).  (Replicating the image rows to 16 and averaging afterwards differs when H is
//   even and no multiple of 16.)  Luma is replicated to 8 ceil(H/8) x 8 ceil(W/8).
//
//   DCT (jfdctint, ISLOW, CONST_BITS 13, PASS1_BITS 2): the 8 rows first, then the 8 columns.
//   One 8-point pass on d0..d7, D(x, n) = (x + 2^(n-1)) >> n:
//     t0..t3 = d0+d7  d1+d6  d2+d5  d3+d4;   t7..t4 = d0-d7  d1-d6  d2-d5  d3-d4
//     t10 = t0+t3;  t13 = t0-t3;  t11 = t1+t2;  t12 = t1-t2
//     rows:     o0 = (t10+t11) << 2;  o4 = (t10-t11) << 2;  s = 11
//     columns:  o0 = D(t10+t11, 2);   o4 = D(t10-t11, 2);   s = 15
//     z1 = (t12+t13) * 4433;  o2 = D(z1 + t13 * 6270, s);  o6 = D(z1 - t12 * 15137, s)
//     z1 = t4+t7;  z2 = t5+t6;  z3 = t4+t6;  z4 = t5+t7;  z5 = (z3+z4) * 9633
//     t4 *= 2446;  t5 *= 16819;  t6 *= 25172;  t7 *= 12299
//     z1 *= -7373;  z2 *= -20995;  z3 = z3 * -16069 + z5;  z4 = z4 * -3196 + z5
//     o7 = D(t4+z1+z3, s);  o5 = D(t5+z2+z4, s);  o3 = D(t6+z2+z3, s);  o1 = D(t7+z1+z4, s)
//   The result is 8 x the DCT coefficient, quantised as in the byte contract.  The AC clamp
//   +-1023 stays as a guard and never fires: the largest |AC| of 8-bit samples is 1020 at q 100.
//
//   Dummy blocks (4:2:0).  A luma block of an MCU whose block row is >= ceil(H/8) or whose block
//   column is >= ceil(W/8) is not transformed: all its AC values are 0 and its DC is the quantised
//   DC of the previous block of the same MCU in the order Y00 Y01 Y10 Y11, itself a dummy or not
//   (at 1x1, Y01 Y10 Y11 all carry Y00's DC).  Chroma blocks are always real.
//
//   Header (jpeg_format.header(layout="pil")): SOI, APP0, a DQT segment per quantisation table
//   (0, 1), SOF0, a DHT segment per Huffman table (DC0, AC0, DC1, AC1), DRI only with a restart
//   interval, SOS; the same with optimised tables, whose four segments the build kernel writes.
//
// Kernel: jpeg_transform_lj_kernel, the shape of jpeg_transform_kernel (one wave per MCU, samples
// in LDS, a lane owns a row and then a column of a block) with the butterfly above in place of
// DCTM (12 multiplies per 8 points instead of 64) and, after quantisation, the wave-uniform
// dummy-block pass.  Everything behind the coefficient buffer is unchanged.
#include "common.h"
#include "kernels.h"
#include "jpeg_fdct_lj.h"
#include "jpeg_entropy_dec.h"
#include "jpeg_entropy_sync.h"
#include "jpeg_entropy_blk.h"
#include "jpeg_huff_opt.h"

namespace {

__constant__ const int DCTM[8][8] = {
  { 2896,  2896,  2896,  2896,  2896,  2896,  2896,  2896},
  { 4017,  3406,  2276,   799,  -799, -2276, -3406, -4017},
  { 3784,  1567, -1567, -3784, -3784, -1567,  1567,  3784},
  { 3406,  -799, -4017, -2276,  2276,  4017,   799, -3406},
  { 2896, -2896, -2896,  2896,  2896, -2896, -2896,  2896},
  { 2276, -4017,   799,  3406, -3406,  -799,  4017, -2276},
  { 1567, -3784,  3784, -1567, -1567,  3784, -3784,  1567},
  {  799, -2276,  3406, -4017,  4017, -3406,  2276,  -799},
};
// zig-zag position of natural (row-major) coefficient index
__constant__ const unsigned char ZPOS[64] = {
   0,  1,  5,  6, 14, 15, 27, 28,  2,  4,  7, 13, 16, 26, 29, 42,
   3,  8, 12, 17, 25, 30, 41, 43,  9, 11, 18, 24, 31, 40, 44, 53,
  10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
  21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63,
};

constexpr int HUFF_WORDS = 2 * 16 + 2 * 256;   // DC luma, DC chroma, AC luma, AC chroma
constexpr int TR_WAVES = 4;

struct Ycc { int y, cb, cr; };
CM_DEVICE Ycc rgb_to_ycc(const uint8_t* p) {
  const int r = p[0], g = p[1], b = p[2];
  Ycc o;
  o.y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  o.cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  o.cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
  return o;
}

// ---------------------------------------------------------------------------------- transform
// One wave per MCU, TR_WAVES MCUs per block.  The wave converts its MCU into level-shifted
// 8x8 sample blocks in LDS, then lane l < 8*nb owns row (l & 7) of block (l >> 3) for the row
// pass and column (l & 7) for the column pass; quantised values go back to LDS at their zig-zag
// position and leave as packed dwords.
template <bool S420>
__global__ __launch_bounds__(64 * TR_WAVES) void jpeg_transform_kernel(JpegArgs a) {
  constexpr int NB = S420 ? 6 : 3;
  __shared__ int sm[TR_WAVES][NB * 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int mcus = a.mx * a.my;
  const long long g = (long long)blockIdx.x * TR_WAVES + wave;
  const bool valid = g < (long long)a.B * mcus;
  int* s = sm[wave];
  if (valid) {
    const int b = (int)(g / mcus), m = (int)(g % mcus);
    const int y0 = (m / a.mx) * (S420 ? 16 : 8), x0 = (m % a.mx) * (S420 ? 16 : 8);
    const uint8_t* img = a.img + (long long)b * a.H * a.W * 3;
    if (S420) {
      const int qy = lane >> 3, qx = lane & 7;
      int cb = 2, cr = 2;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int yy = 2 * qy + (d >> 1), xx = 2 * qx + (d & 1);
        const int y = min(y0 + yy, a.H - 1), x = min(x0 + xx, a.W - 1);
        const Ycc c = rgb_to_ycc(img + ((long long)y * a.W + x) * 3);
        s[((yy >> 3) * 2 + (xx >> 3)) * 64 + (yy & 7) * 8 + (xx & 7)] = c.y - 128;
        cb += c.cb;
        cr += c.cr;
      }
      s[4 * 64 + lane] = (cb >> 2) - 128;
      s[5 * 64 + lane] = (cr >> 2) - 128;
    } else {
      const int y = min(y0 + (lane >> 3), a.H - 1), x = min(x0 + (lane & 7), a.W - 1);
      const Ycc c = rgb_to_ycc(img + ((long long)y * a.W + x) * 3);
      s[lane] = c.y - 128;
      s[64 + lane] = c.cb - 128;
      s[128 + lane] = c.cr - 128;
    }
  }
  __syncthreads();
  const bool worker = valid && lane < NB * 8;
  if (worker) {                       // rows
    int* row = s + lane * 8;
    int x[8], t[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = row[n];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int acc = 1 << 8;
#pragma unroll
      for (int n = 0; n < 8; ++n) acc += DCTM[k][n] * x[n];
      t[k] = acc >> 9;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = t[k];
  }
  __syncthreads();
  int v[8];
  const int blk = lane >> 3, col = lane & 7;
  if (worker) {                       // columns + quantisation
    int x[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = s[blk * 64 + n * 8 + col];
    const int* q = a.qtab + (blk < NB - 2 ? 0 : 64);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int acc = 1 << 13;
#pragma unroll
      for (int n = 0; n < 8; ++n) acc += DCTM[k][n] * x[n];
      const int f = acc >> 14;
      const int q8 = q[k * 8 + col] << 3;
      int mag = (abs(f) + (q8 >> 1)) / q8;
      if (k * 8 + col != 0) mag = min(mag, 1023);
      v[k] = f < 0 ? -mag : mag;
    }
  }
  __syncthreads();
  if (worker) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s[blk * 64 + ZPOS[k * 8 + col]] = v[k];
  }
  __syncthreads();
  if (valid) {
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.coef + g * (NB * 64));
    for (int i = lane; i < NB * 32; i += 64)
      dst[i] = ((uint32_t)s[2 * i] & 0xffffu) | ((uint32_t)s[2 * i + 1] << 16);
  }
}

// ---------------------------------------------------------------------------------- libjpeg transform
// The LIBJPEG FORWARD CONTRACT in the shape of jpeg_transform_kernel.  Row r of block b lies at
// LDS word lj_row(b, r): the rows of a block are rotated by the block's index, so that the column
// pass, where the lanes of a 32-lane half hold the same row of four blocks, reads four different
// banks (ds_read_b32: bank = word mod 32) instead of one four times; a row stays 8 consecutive,
// 32-byte aligned words for the row pass.
CM_DEVICE int lj_row(int b, int r) { return b * 64 + (((r + b) & 7) << 3); }

template <bool S420>
__global__ __launch_bounds__(64 * TR_WAVES) void jpeg_transform_lj_kernel(JpegArgs a) {
  constexpr int NB = S420 ? 6 : 3;
  __shared__ int sm[TR_WAVES][NB * 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int mcus = a.mx * a.my;
  const long long g = (long long)blockIdx.x * TR_WAVES + wave;
  const bool valid = g < (long long)a.B * mcus;
  int* s = sm[wave];
  int mby = 0, mbx = 0;
  if (valid) {
    const int b = (int)(g / mcus), m = (int)(g % mcus);
    mby = m / a.mx;
    mbx = m % a.mx;
    const uint8_t* img = a.img + (long long)b * a.H * a.W * 3;
    if (S420) {
      const int qy = lane >> 3, qx = lane & 7;
      const int y0 = mby * 16, x0 = mbx * 16;
      int cy[2];
      jpeg_lj_chroma_rows(mby * 8 + qy, a.H, cy[0], cy[1]);
      int cb = 0, cr = 0;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int yy = 2 * qy + (d >> 1), xx = 2 * qx + (d & 1);
        const int y = jpeg_lj_src(y0 + yy, a.H), x = jpeg_lj_src(x0 + xx, a.W);
        JpegLjYcc c = jpeg_lj_ycc(img + ((long long)y * a.W + x) * 3);
        s[lj_row((yy >> 3) * 2 + (xx >> 3), yy & 7) + (xx & 7)] = c.y - 128;
        // below the last real chroma row the mean is that row's again, not the luma rows' own
        if (cy[d >> 1] != y) c = jpeg_lj_ycc(img + ((long long)cy[d >> 1] * a.W + x) * 3);
        cb += c.cb;
        cr += c.cr;
      }
      s[lj_row(4, qy) + qx] = jpeg_lj_chroma_mean(cb, qx) - 128;
      s[lj_row(5, qy) + qx] = jpeg_lj_chroma_mean(cr, qx) - 128;
    } else {
      const int r = lane >> 3, c8 = lane & 7;
      const int y = jpeg_lj_src(mby * 8 + r, a.H), x = jpeg_lj_src(mbx * 8 + c8, a.W);
      const JpegLjYcc c = jpeg_lj_ycc(img + ((long long)y * a.W + x) * 3);
      s[lj_row(0, r) + c8] = c.y - 128;
      s[lj_row(1, r) + c8] = c.cb - 128;
      s[lj_row(2, r) + c8] = c.cr - 128;
    }
  }
  __syncthreads();
  const bool worker = valid && lane < NB * 8;
  const int blk = lane >> 3, col = lane & 7;
  if (worker) {                       // rows
    int* row = s + lj_row(blk, col);
    int x[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = row[n];
    jpeg_lj_fdct8<true>(x);
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = x[k];
  }
  __syncthreads();
  int v[8];
  if (worker) {                       // columns + quantisation
#pragma unroll
    for (int n = 0; n < 8; ++n) v[n] = s[lj_row(blk, n) + col];
    jpeg_lj_fdct8<false>(v);
    const int* q = a.qtab + (blk < NB - 2 ? 0 : 64);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = jpeg_lj_quant(v[k], q[k * 8 + col], k * 8 + col != 0);
  }
  __syncthreads();
  if (worker) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s[blk * 64 + ZPOS[k * 8 + col]] = v[k];
  }
  __syncthreads();
  if (S420 && valid) {                // dummy luma blocks: the tests are the same in every lane of the wave
    int dc = s[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if (jpeg_lj_dummy(k, mby, mbx, a.H, a.W)) s[k * 64 + lane] = lane == 0 ? dc : 0;
      else dc = s[k * 64];
    }
  }
  __syncthreads();
  if (valid) {
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.coef + g * (NB * 64));
    for (int i = lane; i < NB * 32; i += 64)
      dst[i] = ((uint32_t)s[2 * i] & 0xffffu) | ((uint32_t)s[2 * i + 1] << 16);
  }
}

// the forward transform a.lj selects, one wave per MCU
static void launch_jpeg_transform(const JpegArgs& a, hipStream_t s) {
  const long long mcus = (long long)a.B * a.mx * a.my;
  const unsigned tg = (unsigned)((mcus + TR_WAVES - 1) / TR_WAVES);
  if (a.lj) {
    if (a.nb == 6) hipLaunchKernelGGL(jpeg_transform_lj_kernel<true>, dim3(tg), dim3(64 * TR_WAVES), 0, s, a);
    else hipLaunchKernelGGL(jpeg_transform_lj_kernel<false>, dim3(tg), dim3(64 * TR_WAVES), 0, s, a);
    return;
  }
  if (a.nb == 6) hipLaunchKernelGGL(jpeg_transform_kernel<true>, dim3(tg), dim3(64 * TR_WAVES), 0, s, a);
  else hipLaunchKernelGGL(jpeg_transform_kernel<false>, dim3(tg), dim3(64 * TR_WAVES), 0, s, a);
}

// ---------------------------------------------------------------------------------- entropy coder
// The count and the write pass run this one coder, so their byte counts cannot differ.
template <bool WRITE>
struct ByteSink {
  uint64_t acc = 0;      // only the low `n` bits are pending
  int n = 0;
  uint32_t pos = 0;
  uint8_t* out = nullptr;
  CM_DEVICE void byte(uint32_t b) {
    if (WRITE) out[pos] = (uint8_t)b;
    ++pos;
  }
  CM_DEVICE void put(uint32_t bits, int len) {     // len <= 27, bits < 2^len
    acc = (acc << len) | bits;
    n += len;
    while (n >= 8) {
      const uint32_t b = (uint32_t)(acc >> (n - 8)) & 0xffu;
      byte(b);
      if (b == 0xffu) byte(0);
      n -= 8;
    }
  }
};

template <bool WRITE>
CM_DEVICE void put_ac(ByteSink<WRITE>& w, const uint32_t* ac, int& run, int val) {
  if (val == 0) {
    ++run;
    return;
  }
  while (run >= 16) {
    const uint32_t z = ac[0xF0];
    w.put(z & 0xffffu, (int)(z >> 16));
    run -= 16;
  }
  const int cat = 32 - __clz(abs(val));
  const uint32_t bits = (uint32_t)(val < 0 ? val - 1 : val) & ((1u << cat) - 1u);
  const uint32_t h = ac[(run << 4) | cat];
  w.put(((h & 0xffffu) << cat) | bits, (int)(h >> 16) + cat);
  run = 0;
}

// Optimised tables: the image's own words and header length (a.ihuff is null with the standard
// tables, and then every image shares a.huff and a.hdr_len).
CM_DEVICE const uint32_t* image_huff(const JpegArgs& a, int b) {
  return a.ihuff != nullptr ? a.ihuff + (long long)b * HUFF_WORDS : reinterpret_cast<const uint32_t*>(a.huff);
}
CM_DEVICE uint32_t image_hdr_len(const JpegArgs& a, int b) {
  return a.ihuff != nullptr ? a.hdr_lens[b] : (uint32_t)a.hdr_len;
}

// one lane per restart interval (gid = image * nint + interval); with optimised tables
// blockIdx.y is the image and blockIdx.x tiles its intervals
template <bool WRITE>
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(JpegArgs a) {
  __shared__ uint32_t huff[HUFF_WORDS];
  const bool per_image = a.ihuff != nullptr;
  const uint32_t* hsrc = image_huff(a, per_image ? (int)blockIdx.y : 0);
  for (int i = threadIdx.x; i < HUFF_WORDS; i += 64) huff[i] = hsrc[i];
  __syncthreads();
  long long gid = (long long)blockIdx.x * 64 + threadIdx.x;
  if (per_image) {
    if (gid >= a.nint) return;
    gid += (long long)blockIdx.y * a.nint;
  }
  if (gid >= (long long)a.B * a.nint) return;
  const int b = (int)(gid / a.nint), it = (int)(gid % a.nint);
  const int mcus = a.mx * a.my;
  const int m0 = it * a.restart, m1 = min(m0 + a.restart, mcus);
  ByteSink<WRITE> w;
  if (WRITE) w.out = a.out + a.base[b] + image_hdr_len(a, b) + a.offs[gid];
  const uint4* p = reinterpret_cast<const uint4*>(a.coef + ((long long)b * mcus + m0) * a.nb * 64);
  int p0 = 0, p1 = 0, p2 = 0;
  for (int m = m0; m < m1; ++m) {
    for (int blk = 0; blk < a.nb; ++blk, p += 8) {
      const int comp = blk < a.nb - 2 ? 0 : blk - (a.nb - 2) + 1;
      const uint32_t* dc = huff + (comp == 0 ? 0 : 16);
      const uint32_t* ac = huff + 32 + (comp == 0 ? 0 : 256);
      int run = 0;
#pragma unroll 1
      for (int c = 0; c < 8; ++c) {
        const uint4 q = p[c];
        const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
        if (c == 0) {
          const int v0 = (short)(wd[0] & 0xffffu);
          const int pred = comp == 0 ? p0 : (comp == 1 ? p1 : p2);
          const int d = v0 - pred;
          if (comp == 0) p0 = v0; else if (comp == 1) p1 = v0; else p2 = v0;
          const int cat = 32 - __clz(abs(d));            // 0 for d == 0
          const uint32_t bits = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << cat) - 1u);
          const uint32_t h = dc[cat];
          w.put(((h & 0xffffu) << cat) | bits, (int)(h >> 16) + cat);
          put_ac(w, ac, run, (int)(short)(wd[0] >> 16));
#pragma unroll
          for (int j = 2; j < 8; ++j) put_ac(w, ac, run, (int)(short)((wd[j >> 1] >> (16 * (j & 1))) & 0xffffu));
        } else if ((q.x | q.y | q.z | q.w) == 0u) {
          run += 8;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) put_ac(w, ac, run, (int)(short)((wd[j >> 1] >> (16 * (j & 1))) & 0xffffu));
        }
      }
      if (run > 0) w.put(ac[0] & 0xffffu, (int)(ac[0] >> 16));   // EOB
    }
  }
  if (w.n > 0) w.put((1u << (8 - w.n)) - 1u, 8 - w.n);
  w.byte(0xff);
  w.byte(it + 1 < a.nint ? 0xD0u + (uint32_t)(it & 7) : 0xD9u);
  if (!WRITE) a.lens[gid] = w.pos;
}

// ---------------------------------------------------------------------------------- scans
CM_DEVICE uint32_t wave_inclusive_scan(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(v, o, 64);
    if (lane >= o) v += y;
  }
  return v;
}

// per image: offs = exclusive scan of lens; base[1 + image] = header + entropy bytes of the image
__global__ __launch_bounds__(256) void jpeg_scan_image_kernel(JpegArgs a) {
  __shared__ uint32_t wsum[4];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t* lens = a.lens + (long long)b * a.nint;
  uint32_t* offs = a.offs + (long long)b * a.nint;
  uint32_t running = 0;
  for (int i0 = 0; i0 < a.nint; i0 += 256) {
    const int i = i0 + tid;
    const uint32_t v = i < a.nint ? lens[i] : 0u;
    const uint32_t inc = wave_inclusive_scan(v, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < wave) pre += wsum[k];
      tot += wsum[k];
    }
    if (i < a.nint) offs[i] = running + pre + inc - v;
    running += tot;
    __syncthreads();
  }
  if (tid == 0) a.base[1 + b] = image_hdr_len(a, b) + running;
}

// over the batch, one wave: base[1 + i] (image sizes) -> inclusive scan in place, base[0] = 0
__global__ __launch_bounds__(64) void jpeg_scan_batch_kernel(JpegArgs a) {
  const int lane = threadIdx.x;
  uint32_t running = 0;
  for (int i0 = 0; i0 < a.B; i0 += 64) {
    const int i = i0 + lane;
    const uint32_t v = i < a.B ? a.base[1 + i] : 0u;
    const uint32_t inc = wave_inclusive_scan(v, lane);
    if (i < a.B) a.base[1 + i] = running + inc;
    running += __shfl(inc, 63, 64);
  }
  if (lane == 0) a.base[0] = 0;
}

__global__ __launch_bounds__(256) void jpeg_header_kernel(JpegArgs a) {
  uint8_t* dst = a.out + a.base[blockIdx.x];
  if (a.ihuff != nullptr) {                              // the image's own header, built with its tables
    const uint8_t* src = a.hdrs + (long long)blockIdx.x * a.hdr_cap;
    const int n = min((int)a.hdr_lens[blockIdx.x], a.hdr_cap);
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
    return;
  }
  for (int i = threadIdx.x; i < a.hdr_len; i += 256) dst[i] = a.header[i];
}

// ---------------------------------------------------------------------------------- optimised Huffman tables
constexpr int HUFF_BASE[4] = {0, 16, 32, 32 + 256};    // DC luma, DC chroma, AC luma, AC chroma in HUFF_WORDS
constexpr int HUFF_COUNT_LANES = 256;                   // = BLK_LANES: the geometry of the bits kernel

// One lane per block of image blockIdx.y: the coder's symbol walk with the counting sink into the
// workgroup's LDS histogram, then one integer atomicAdd per non-zero word into freq[image].
__global__ __launch_bounds__(HUFF_COUNT_LANES) void jpeg_huff_count_kernel(JpegArgs a) {
  __shared__ uint32_t hist[HUFF_WORDS];
  for (int i = threadIdx.x; i < HUFF_WORDS; i += HUFF_COUNT_LANES) hist[i] = 0u;
  __syncthreads();
  const long long per_img = (long long)a.mx * a.my * a.nb;
  const long long r = (long long)blockIdx.x * HUFF_COUNT_LANES + threadIdx.x;
  const int b = blockIdx.y;
  if (r < per_img) {
    const long long m = r / a.nb;
    const int blk = (int)(r % a.nb);
    const int16_t* img = a.coef + (long long)b * per_img * 64;
    const bool luma = blk < a.nb - 2;
    jpeg_blk_count(img + r * 64, jpeg_blk_pred(img, m, blk, a.nb, a.restart), hist + (luma ? 0 : 16),
                   hist + 32 + (luma ? 0 : 256));
  }
  __syncthreads();
  uint32_t* freq = a.freq + (long long)b * HUFF_WORDS;
  for (int i = threadIdx.x; i < HUFF_WORDS; i += HUFF_COUNT_LANES)
    if (hist[i] != 0u) atomicAdd(freq + i, hist[i]);
}

// One workgroup per image, wave t builds table t (jpeg_huff_opt.h) in LDS; then the workgroup
// writes the image's code words, its header and its header length (0: a table was refused).
__global__ __launch_bounds__(256) void jpeg_huff_build_kernel(JpegArgs a) {
  __shared__ JpegHuffWork work[4];
  const int b = blockIdx.x, tid = threadIdx.x, t = tid >> 6, lane = tid & 63;
  const int base = t == 0 ? HUFF_BASE[0] : (t == 1 ? HUFF_BASE[1] : (t == 2 ? HUFF_BASE[2] : HUFF_BASE[3]));
  const int nslots = t < 2 ? 16 : 256;
  JpegHuffWork& w = work[t];
  const uint32_t* freq = a.freq + (long long)b * HUFF_WORDS + base;
  for (int i = lane; i < JPEG_HUFF_SYMS; i += 64) w.freq[i] = i < nslots ? freq[i] : 0u;
  jpeg_huff_sync();
  jpeg_huff_build(w, lane);
  jpeg_huff_assign(w, a.ihuff + (long long)b * HUFF_WORDS + base, nslots, lane);
  __syncthreads();
  const int pre = a.hdr_split, suf = a.hdr_len - a.hdr_split;
  uint8_t* dst = a.hdrs + (long long)b * a.hdr_cap;
  for (int i = tid; i < pre; i += 256) dst[i] = a.header[i];
  const uint32_t room = (uint32_t)max(a.hdr_cap - pre - suf, 0);
  const uint32_t dht = jpeg_huff_dht(work, dst + pre, room, tid, 256, a.lj != 0);
  const bool ok = dht <= room && (work[0].bad | work[1].bad | work[2].bad | work[3].bad) == 0u;
  if (ok)
    for (int i = tid; i < suf; i += 256) dst[pre + dht + i] = a.header[pre + i];
  if (tid == 0) a.hdr_lens[b] = ok ? (uint32_t)pre + dht + (uint32_t)suf : 0u;
}

// ---------------------------------------------------------------------------------- reconstruct
// natural (row-major) coefficient index of zig-zag position (the inverse of ZPOS)
__constant__ const unsigned char ZNAT[64] = {
   0,  1,  8, 16,  9,  2,  3, 10, 17, 24, 32, 25, 18, 11,  4,  5,
  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,  6,  7, 14, 21, 28,
  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
  58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
};

// one 8-point pass of the inverse DCT of the decode contract, in place; S = its descale shift
template <int S>
CM_DEVICE void idct_pass(int (&x)[8]) {
  int z1 = (x[2] + x[6]) * 4433;
  const int t2 = z1 - x[6] * 15137, t3 = z1 + x[2] * 6270;
  const int t0 = (x[0] + x[4]) * 8192, t1 = (x[0] - x[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a = x[7], b = x[5], c = x[3], d = x[1];
  z1 = a + d;
  int z2 = b + c, z3 = a + c, z4 = b + d;
  const int z5 = (z3 + z4) * 9633;
  a *= 2446; b *= 16819; c *= 25172; d *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  a += z1 + z3; b += z2 + z4; c += z2 + z3; d += z1 + z4;
  constexpr int half = 1 << (S - 1);
  x[0] = (t10 + d + half) >> S; x[7] = (t10 - d + half) >> S;
  x[1] = (t11 + c + half) >> S; x[6] = (t11 - c + half) >> S;
  x[2] = (t12 + b + half) >> S; x[5] = (t12 - b + half) >> S;
  x[3] = (t13 + a + half) >> S; x[4] = (t13 - a + half) >> S;
}

// LDS image of one MCU: sample (row r, column c) of block k at k * ID_BLK + r * ID_ROW + c.  The
// odd row stride keeps both passes free of bank conflicts (lane = 8 k + column, then 8 k + row).
constexpr int ID_ROW = 9, ID_BLK = 8 * ID_ROW;

// One wave per MCU, TR_WAVES MCUs per block.  The wave unpacks its MCU's coefficients into LDS at
// their natural position, dequantised; lane l < 8*nb owns column (l & 7) of block (l >> 3) for
// the column pass and row (l & 7) for the row pass; the samples leave as packed dwords into the
// padded planes: Y [B][yh][yw], then Cb [B][8 my][8 mx], then Cr (yh x yw = 16 my x 16 mx for
// 420, 8 my x 8 mx for 444).
template <bool S420>
__global__ __launch_bounds__(64 * TR_WAVES) void jpeg_idct_kernel(JpegArgs a) {
  constexpr int NB = S420 ? 6 : 3;
  __shared__ int sm[TR_WAVES][NB * ID_BLK];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int mcus = a.mx * a.my;
  const long long g = (long long)blockIdx.x * TR_WAVES + wave;
  const bool valid = g < (long long)a.B * mcus;
  int* s = sm[wave];
  if (valid) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.coef + g * (NB * 64));
    for (int i = lane; i < NB * 32; i += 64) {
      const uint32_t w = src[i];
      const int blk = i >> 5, z = (2 * i) & 63;
      const int* q = a.qtab + (blk < NB - 2 ? 0 : 64);
      const int n0 = ZNAT[z], n1 = ZNAT[z + 1];
      s[blk * ID_BLK + (n0 >> 3) * ID_ROW + (n0 & 7)] = (int)(short)(w & 0xffffu) * q[n0];
      s[blk * ID_BLK + (n1 >> 3) * ID_ROW + (n1 & 7)] = (int)(short)(w >> 16) * q[n1];
    }
  }
  __syncthreads();
  const bool worker = valid && lane < NB * 8;
  const int blk = lane >> 3, own = lane & 7;
  if (worker) {                       // columns
    int* col = s + blk * ID_BLK + own;
    int x[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = col[n * ID_ROW];
    idct_pass<11>(x);
#pragma unroll
    for (int n = 0; n < 8; ++n) col[n * ID_ROW] = x[n];
  }
  __syncthreads();
  if (worker) {                       // rows, level shift, clamp
    int* row = s + blk * ID_BLK + own * ID_ROW;
    int x[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = row[n];
    idct_pass<18>(x);
#pragma unroll
    for (int n = 0; n < 8; ++n) row[n] = min(max(x[n] + 128, 0), 255);
  }
  __syncthreads();
  if (valid) {
    const int b = (int)(g / mcus), m = (int)(g % mcus);
    const int my0 = m / a.mx, mx0 = m % a.mx;
    const long long csz = (long long)mcus * 64;                 // bytes of one 8 my x 8 mx plane
    const int cw = a.mx * 8;
    if (S420) {                       // Y: 16 rows x 4 dwords
      const int r = lane >> 2, xq = (lane & 3) * 4;
      const int* p = s + ((r >> 3) * 2 + (xq >> 3)) * ID_BLK + (r & 7) * ID_ROW + (xq & 7);
      uint8_t* dst = a.planes + ((long long)b * a.my * 16 + my0 * 16 + r) * (cw * 2) + mx0 * 16 + xq;
      *reinterpret_cast<uint32_t*>(dst) = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    // 8x8 planes, 16 lanes each: Cb, Cr (420, after the Y planes) or Y, Cb, Cr (444)
    constexpr int NP = S420 ? 2 : 3;
    if (lane < NP * 16) {
      const int pl = lane >> 4, r = (lane & 15) >> 1, xq = (lane & 1) * 4;
      const int* p = s + (pl + NB - NP) * ID_BLK + r * ID_ROW + xq;
      uint8_t* base = a.planes + (S420 ? 4 * csz * a.B : 0) + pl * csz * a.B;
      uint8_t* dst = base + ((long long)b * a.my * 8 + my0 * 8 + r) * cw + mx0 * 8 + xq;
      *reinterpret_cast<uint32_t*>(dst) = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
  }
}

CM_DEVICE int clamp8(int v) { return min(max(v, 0), 255); }

// One lane per run of 4 output pixels (x0 = 4 k): one dword of Y, the chroma samples it needs
// (420: up to 2 rows x 4 columns per plane, indices clamped to the real samples), 12 bytes out.
template <bool S420>
__global__ __launch_bounds__(256) void jpeg_colour_kernel(JpegArgs a) {
  const int xg = (a.W + 3) >> 2;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)a.B * a.H * xg) return;
  const int x0 = (int)(gid % xg) * 4;
  const long long line = gid / xg;                   // b * H + y
  const int y = (int)(line % a.H), b = (int)(line / a.H);
  const int cwp = a.mx * 8, chp = a.my * 8;          // padded 8 my x 8 mx plane
  const int yw = S420 ? cwp * 2 : cwp, yh = S420 ? chp * 2 : chp;
  const uint8_t* cbp = a.planes + (long long)a.B * yh * yw + (long long)b * chp * cwp;
  const uint8_t* crp = cbp + (long long)a.B * chp * cwp;
  const uint32_t yy = *reinterpret_cast<const uint32_t*>(a.planes + ((long long)b * yh + y) * yw + x0);
  int cb[4], cr[4];
  if (S420) {
    const int ch = (a.H + 1) >> 1, cw = (a.W + 1) >> 1;
    const int r = y >> 1, cx = x0 >> 1;
    const uint8_t* b0 = cbp + (long long)r * cwp;
    const uint8_t* r0 = crp + (long long)r * cwp;
    if (cw <= 2) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = min(cx + (j >> 1), cw - 1);
        cb[j] = b0[c];
        cr[j] = r0[c];
      }
    } else {
      const long long dn = (long long)(min(max((y & 1) ? r + 1 : r - 1, 0), ch - 1) - r) * cwp;
      int sb[4], sr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = min(max(cx - 1 + j, 0), cw - 1);
        sb[j] = 3 * b0[c] + b0[dn + c];
        sr[j] = 3 * r0[c] + r0[dn + c];
      }
      cb[0] = (3 * sb[1] + sb[0] + 8) >> 4; cr[0] = (3 * sr[1] + sr[0] + 8) >> 4;
      cb[1] = (3 * sb[1] + sb[2] + 7) >> 4; cr[1] = (3 * sr[1] + sr[2] + 7) >> 4;
      cb[2] = (3 * sb[2] + sb[1] + 8) >> 4; cr[2] = (3 * sr[2] + sr[1] + 8) >> 4;
      cb[3] = (3 * sb[2] + sb[3] + 7) >> 4; cr[3] = (3 * sr[2] + sr[3] + 7) >> 4;
    }
  } else {
    const long long o = (long long)y * cwp + x0;
    const uint32_t wb = *reinterpret_cast<const uint32_t*>(cbp + o);
    const uint32_t wr = *reinterpret_cast<const uint32_t*>(crp + o);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cb[j] = (int)((wb >> (8 * j)) & 0xffu);
      cr[j] = (int)((wr >> (8 * j)) & 0xffu);
    }
  }
  uint32_t px[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int Y = (int)((yy >> (8 * j)) & 0xffu), u = cb[j] - 128, v = cr[j] - 128;
    px[3 * j] = (uint32_t)clamp8(Y + ((91881 * v + 32768) >> 16));
    px[3 * j + 1] = (uint32_t)clamp8(Y + ((-22554 * u - 46802 * v + 32768) >> 16));
    px[3 * j + 2] = (uint32_t)clamp8(Y + ((116130 * u + 32768) >> 16));
  }
  uint8_t* dst = a.dec + (line * a.W + x0) * 3;
  if ((a.W & 3) == 0) {               // rows are dword-aligned and whole: three dword stores
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | (px[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (x0 + j / 3 < a.W) dst[j] = (uint8_t)px[j];
  }
}

// ---------------------------------------------------------------------------------- entropy decode
// one lane per restart interval (gid = image * nint + interval), the mirror of jpeg_entropy_kernel.
// Lanes diverge by design (every interval is its own bit stream); the per-lane state is the bit
// window, three predictors and a few scalars, no indexed register arrays.
__global__ __launch_bounds__(64) void jpeg_entropy_decode_kernel(JpegArgs a, JpegDecodeIn d) {
  __shared__ uint32_t tabs[JPEG_DEC_WORDS];
  for (int i = threadIdx.x; i < JPEG_DEC_WORDS; i += 64) tabs[i] = d.tables[i];
  __syncthreads();
  const long long gid = (long long)blockIdx.x * 64 + threadIdx.x;
  if (gid >= (long long)a.B * a.nint) return;
  const int b = (int)(gid / a.nint), it = (int)(gid % a.nint);
  const int mcus = a.mx * a.my;
  const int m0 = it * a.restart;
  const uint32_t off = d.intervals[2 * gid], len = d.intervals[2 * gid + 1];
  int st;
  if (m0 >= mcus) {
    st = JPEG_DEC_OVERRUN;
  } else if (off > d.nbytes || len > d.nbytes - off) {
    st = JPEG_DEC_TRUNCATED;
  } else {
    st = jpeg_decode_interval(d.bytes + off, len, tabs, a.nb, min(a.restart, mcus - m0),
                              a.coef + ((long long)b * mcus + m0) * a.nb * 64);
  }
  // the error of the lowest gid wins: larger key = smaller gid; 0 = every interval OK
  if (st != JPEG_DEC_OK)
    atomicMax(d.status, ((unsigned long long)(0xffffffffu - (uint32_t)gid) << 32) | (unsigned long long)st);
}

// ---------------------------------------------------------------------------------- chunked entropy decode
// Inclusive scan of one word per thread over the block (Hillis-Steele, buf = 2 * N words of LDS).
// Every thread of the block calls it; the barriers are block-uniform.
template <int N>
CM_DEVICE uint32_t jpeg_block_scan(uint32_t v, uint32_t* buf) {
  const int t = threadIdx.x, n = blockDim.x;
  int cur = 0;
  buf[t] = v;
  __syncthreads();
  for (int dlt = 1; dlt < n; dlt <<= 1) {
    uint32_t x = buf[cur * N + t];
    if (t >= dlt) x += buf[cur * N + t - dlt];
    buf[(cur ^ 1) * N + t] = x;
    __syncthreads();
    cur ^= 1;
  }
  const uint32_t r = buf[cur * N + t];
  __syncthreads();                     // buf is free again
  return r;
}

// One lane per chunk, one workgroup per group of consecutive intervals (y.groups).  Thread t is
// lane t of the group; its interval is the last one whose first lane (y.lane0) is <= t.  Threads
// past the last chunk stay idle but take every barrier: nothing returns before the last one, and
// every loop around a barrier has a block-uniform condition (an LDS word read after a barrier,
// blockDim).
__global__ __launch_bounds__(JPEG_SYNC_MAX_CHUNKS) void jpeg_entropy_sync_kernel(JpegArgs a, JpegDecodeIn d, JpegSyncIn y) {
  constexpr int N = JPEG_SYNC_MAX_CHUNKS;
  __shared__ uint32_t tabs[JPEG_DEC_WORDS];
  __shared__ uint32_t sl0[N], sexit[N], sbuf[2 * N];
  __shared__ uint32_t sany[2];
  const int t = threadIdx.x, n = blockDim.x;
  for (int i = t; i < JPEG_DEC_WORDS; i += n) tabs[i] = d.tables[i];
  const long long nivals = (long long)a.B * a.nint;
  const long long g0 = y.groups[2 * blockIdx.x];
  uint32_t gn = y.groups[2 * blockIdx.x + 1];
  if (g0 >= nivals) gn = 0;
  else if (gn > nivals - g0) gn = (uint32_t)(nivals - g0);
  if (gn > (uint32_t)N) gn = N;
  for (uint32_t i = t; i < gn; i += n) sl0[i] = y.lane0[g0 + i];
  if (t == 0) sany[0] = sany[1] = 0;
  __syncthreads();

  // this lane's interval and chunk
  bool active = false;
  uint32_t l0 = 0, len = 0, begin = 0, end = 0;
  const uint8_t* bytes = d.bytes;
  int16_t* coef = a.coef;
  int nblk = 0;
  if (gn > 0) {
    uint32_t lo = 0, hi = gn;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (sl0[mid] <= (uint32_t)t) lo = mid; else hi = mid;
    }
    l0 = sl0[lo];
    const long long gid = g0 + lo;
    const int b = (int)(gid / a.nint), it = (int)(gid % a.nint);
    const int mcus = a.mx * a.my;
    const long long m0 = (long long)it * a.restart;
    const uint32_t off = d.intervals[2 * gid], ln = d.intervals[2 * gid + 1];
    if (l0 <= (uint32_t)t && l0 < (uint32_t)n) {
      const uint32_t c = (uint32_t)t - l0;
      const unsigned long long bg = (unsigned long long)c * y.cb;
      if (m0 >= mcus || off > d.nbytes || ln > d.nbytes - off || ln >= JPEG_SYNC_MAX_LEN) {
        if (c == 0) atomicOr(y.words, 1u);                     // the serial kernel names the error
      } else if (bg < ln) {
        active = true;
        len = ln;
        begin = (uint32_t)bg;
        end = (uint32_t)min((unsigned long long)ln, bg + y.cb);
        bytes = d.bytes + off;
        nblk = (int)min((long long)a.restart, mcus - m0) * a.nb;
        coef = a.coef + ((long long)b * mcus + m0) * a.nb * 64;
      }
    }
  }
  const bool head = begin == 0;          // lane 0 of its interval: its start is the truth
  uint32_t start = active && !head ? jpeg_sync_pack(jpeg_sync_guess(bytes, len, begin), 0, 0, begin) : 0u;
  uint32_t blocks = 0;
  bool run = active;
  sexit[t] = JPEG_SYNC_ERR;
  if (run) sany[0] = 1;
  __syncthreads();

  // the rounds
  int rounds = 0;
  for (int r = 0; r < n && sany[r & 1] != 0; ++r) {
    ++rounds;
    if (run) {
      JpegSyncRun s;
      jpeg_sync_unpack(start, begin, s);
      jpeg_sync_lane_run<false>(bytes, len, end, tabs, a.nb, s, 0, 0, nullptr);
      blocks = s.blocks;
      sexit[t] = s.err != JPEG_DEC_OK ? JPEG_SYNC_ERR : jpeg_sync_pack(s.p, s.blk, s.k, end);
    }
    if (t == 0) sany[(r + 1) & 1] = 0;
    __syncthreads();
    run = false;
    if (active && !head) {
      const uint32_t e = sexit[t - 1];                         // !head: t > l0 >= 0
      if (e != JPEG_SYNC_ERR && e != start) {
        start = e;
        run = true;
        sany[(r + 1) & 1] = 1;
      }
    }
    __syncthreads();
  }

  // valid chain: no error exit among the lanes before this one in its interval
  const uint32_t bad = active && sexit[t] == JPEG_SYNC_ERR ? 1u : 0u;
  const uint32_t badx = jpeg_block_scan<N>(bad, sbuf) - bad;
  sl0[t] = badx;                                                // the group's lane0 table is no longer needed
  __syncthreads();
  const bool valid = active && badx == sl0[l0];
  __syncthreads();
  // placement: exclusive scan of the valid lanes' block counts within the interval
  const uint32_t cnt = valid ? blocks : 0u;
  const uint32_t cntx = jpeg_block_scan<N>(cnt, sbuf) - cnt;
  sl0[t] = cntx;
  __syncthreads();
  if (valid) {
    JpegSyncRun s;
    jpeg_sync_unpack(start, begin, s);
    const long long first = (long long)(cntx - sl0[l0]) - (s.k != 0 ? 1 : 0);
    if (first < nblk) {
      jpeg_sync_lane_run<true>(bytes, len, end, tabs, a.nb, s, (int)first, nblk, coef);
      if (s.err != JPEG_DEC_OK && s.err_block < nblk) atomicOr(y.words, 1u);
      if (s.done != 0) atomicAdd(y.words + 2, s.done);
    }
  }
  if (t == 0) atomicMax(y.words + 1, (uint32_t)rounds);
}

// One workgroup per interval (64 .. 1024 threads, as many as the interval has luma blocks): the DC
// differences the write pass stored become the predictors.  A thread owns a run of consecutive
// blocks of the component; its loads are independent, the chain between threads is the scan.
__global__ __launch_bounds__(1024) void jpeg_dc_prefix_kernel(JpegArgs a, JpegDecodeIn d, JpegSyncIn y) {
  __shared__ uint32_t sbuf[2 * 1024];
  const int t = threadIdx.x, n = blockDim.x;
  const long long gid = blockIdx.x;
  const int b = (int)(gid / a.nint), it = (int)(gid % a.nint);
  const int mcus = a.mx * a.my;
  const long long m0 = (long long)it * a.restart;
  if (m0 >= mcus) return;                                       // the whole block: before any barrier
  const int nmcu = (int)min((long long)a.restart, mcus - m0), nb = a.nb;
  int16_t* coef = a.coef + ((long long)b * mcus + m0) * nb * 64;
  for (int comp = 0; comp < 3; ++comp) {
    const int per_mcu = comp == 0 ? nb - 2 : 1;
    const int cnt = nmcu * per_mcu, per = (cnt + n - 1) / n;
    const int lo = min(cnt, t * per), hi = min(cnt, lo + per);
    const uint32_t q0 = d.tables[comp == 0 ? 0 : 64];
    uint32_t sum = 0;
    for (int i = lo; i < hi; ++i) {
      const long long blk = (long long)(i / per_mcu) * nb + (comp == 0 ? i % per_mcu : nb - 3 + comp);
      sum += (uint32_t)(int)coef[blk * 64];
    }
    uint32_t pred = jpeg_block_scan<1024>(sum, sbuf) - sum;
    bool wide = false;
    for (int i = lo; i < hi; ++i) {
      const long long blk = (long long)(i / per_mcu) * nb + (comp == 0 ? i % per_mcu : nb - 3 + comp);
      pred += (uint32_t)(int)coef[blk * 64];
      const bool ok = jpeg_sync_dc_ok(pred, q0);
      coef[blk * 64] = ok ? (int16_t)(int32_t)pred : (int16_t)0;
      wide |= !ok;
    }
    if (wide) atomicOr(y.words, 1u);
  }
}

// One thread per block: the refusal rule on what was stored.
__global__ __launch_bounds__(256) void jpeg_block_check_kernel(JpegArgs a, JpegDecodeIn d, JpegSyncIn y) {
  __shared__ uint32_t q[JPEG_DEC_QZ_WORDS];
  if (threadIdx.x < JPEG_DEC_QZ_WORDS) q[threadIdx.x] = d.tables[threadIdx.x];
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.B * a.mx * a.my * a.nb) return;
  const int blk = (int)(i % a.nb);
  if (!jpeg_sync_block_ok(a.coef + i * 64, q + (blk < a.nb - 2 ? 0 : 64))) atomicOr(y.words, 1u);
}

// ---------------------------------------------------------------------------------- block-parallel entropy coder
constexpr int BLK_LANES = 256;

// One lane per block (g = (image * mcus + MCU) * nb + block): its bit length.  Lanes diverge with
// their blocks' contents (4 .. 1660 bits); the per-lane state is one coefficient chunk and a few
// scalars.
__global__ __launch_bounds__(BLK_LANES) void jpeg_blk_bits_kernel(JpegArgs a, JpegBlkArgs k) {
  __shared__ uint32_t huff[HUFF_WORDS];
  const bool per_image = a.ihuff != nullptr;             // blockIdx.y = image, blockIdx.x tiles its blocks
  const uint32_t* hsrc = image_huff(a, per_image ? (int)blockIdx.y : 0);
  for (int i = threadIdx.x; i < HUFF_WORDS; i += BLK_LANES) huff[i] = hsrc[i];
  __syncthreads();
  const long long per_img = (long long)a.mx * a.my * a.nb;
  long long g = (long long)blockIdx.x * BLK_LANES + threadIdx.x;
  if (per_image) {
    if (g >= per_img) return;
    g += (long long)blockIdx.y * per_img;
  }
  if (g >= (long long)a.B * per_img) return;
  const long long r = g % per_img, m = r / a.nb;
  const int blk = (int)(r % a.nb);
  const int16_t* img = a.coef + (g - r) * 64;
  const bool luma = blk < a.nb - 2;
  JpegBlkSink<false> w;
  jpeg_blk_code<false>(img + r * 64, jpeg_blk_pred(img, m, blk, a.nb, a.restart), huff + (luma ? 0 : 16),
                       huff + 32 + (luma ? 0 : 256), w);
  k.bits[g] = w.pos;
}

// One workgroup per interval (64 .. 1024 threads, tiles of blockDim blocks with a running sum):
// bits[] becomes the exclusive scan of the lengths, ubits the interval's bit count.  Every word a
// block starts in, and the one the interval ends in, is zeroed here: those are the only words the
// pack pass merges into (all others have one writer, which stores).
__global__ __launch_bounds__(1024) void jpeg_blk_scan_kernel(JpegArgs a, JpegBlkArgs k) {
  __shared__ uint32_t sbuf[2 * 1024];
  __shared__ uint32_t stot;
  const int t = threadIdx.x, n = blockDim.x;
  const long long gid = blockIdx.x;
  const int b = (int)(gid / a.nint), it = (int)(gid % a.nint);
  const int mcus = a.mx * a.my;
  const long long m0 = (long long)it * a.restart;
  const int nblk = (int)max(0LL, min((long long)a.restart, mcus - m0)) * a.nb;
  uint32_t* bits = k.bits + ((long long)b * mcus + m0) * a.nb;
  uint32_t* words = k.scratch + gid * k.stride;
  uint32_t running = 0;
  bool bad = false;
  for (int i0 = 0; i0 < nblk; i0 += n) {
    const int i = i0 + t;
    const uint32_t v = i < nblk ? bits[i] : 0u;
    const uint32_t inc = jpeg_block_scan<1024>(v, sbuf);
    if (t == n - 1) stot = inc;
    if (i < nblk) {
      const uint32_t off = running + inc - v;
      bits[i] = off;
      if ((off >> 5) < k.stride) words[off >> 5] = 0u;
      else bad = true;
    }
    __syncthreads();
    running += stot;
    __syncthreads();
  }
  if (t == 0) {
    k.ubits[gid] = running;
    if ((running >> 5) < k.stride) words[running >> 5] = 0u;
    else if ((running >> 5) > k.stride || (running & 31u) != 0u) bad = true;
  }
  if (bad) atomicOr(k.err, 1u);
}

// One lane per block again: the same coder, storing at the block's bit offset.
__global__ __launch_bounds__(BLK_LANES) void jpeg_blk_pack_kernel(JpegArgs a, JpegBlkArgs k) {
  __shared__ uint32_t huff[HUFF_WORDS];
  const bool per_image = a.ihuff != nullptr;             // as in the bits kernel
  const uint32_t* hsrc = image_huff(a, per_image ? (int)blockIdx.y : 0);
  for (int i = threadIdx.x; i < HUFF_WORDS; i += BLK_LANES) huff[i] = hsrc[i];
  __syncthreads();
  const int mcus = a.mx * a.my;
  const long long per_img = (long long)mcus * a.nb;
  long long g = (long long)blockIdx.x * BLK_LANES + threadIdx.x;
  if (per_image) {
    if (g >= per_img) return;
    g += (long long)blockIdx.y * per_img;
  }
  if (g >= (long long)a.B * per_img) return;
  const long long r = g % per_img, m = r / a.nb;
  const int blk = (int)(r % a.nb);
  const int16_t* img = a.coef + (g - r) * 64;
  const bool luma = blk < a.nb - 2;
  const long long it = m / a.restart, gid = (g / per_img) * a.nint + it;
  const bool last = blk == a.nb - 1 && m == min((it + 1) * a.restart, (long long)mcus) - 1;
  const uint32_t off = k.bits[g];
  JpegBlkSink<true> w;
  w.start(k.scratch + gid * k.stride, k.stride, off);
  jpeg_blk_code<true>(img + r * 64, jpeg_blk_pred(img, m, blk, a.nb, a.restart), huff + (luma ? 0 : 16),
                      huff + 32 + (luma ? 0 : 256), w);
  w.finish(off, last);
  if (w.bad) atomicOr(k.err, 1u);
}

// One workgroup per interval, one lane per piece of JPEG_BLK_PIECE unstuffed bytes (tiles of
// blockDim pieces with a running sum): the stuffed length of every piece, its scan, and either the
// interval's length with its marker (lens) or the bytes at their final place.
template <bool WRITE>
__global__ __launch_bounds__(1024) void jpeg_blk_stuff_kernel(JpegArgs a, JpegBlkArgs k) {
  __shared__ uint32_t sbuf[2 * 1024];
  __shared__ uint32_t stot;
  const int t = threadIdx.x, n = blockDim.x;
  const long long gid = blockIdx.x;
  const int b = (int)(gid / a.nint), it = (int)(gid % a.nint);
  const uint32_t* words = k.scratch + gid * k.stride;
  const uint32_t ub = k.ubits[gid];
  uint32_t ubytes = (ub >> 3) + ((ub & 7u) != 0u ? 1u : 0u);
  bool bad = false;
  if (ubytes > 4u * k.stride) {                      // stride < 2^30 (checked by the caller)
    ubytes = 4u * k.stride;
    bad = true;
  }
  const uint32_t npiece = (ubytes + JPEG_BLK_PIECE - 1u) / JPEG_BLK_PIECE;
  const uint32_t dst = WRITE ? a.base[b] + image_hdr_len(a, b) + a.offs[gid] : 0u;
  uint32_t running = 0;
  for (uint32_t p0 = 0; p0 < npiece; p0 += (uint32_t)n) {
    const uint32_t p = p0 + (uint32_t)t;
    const uint32_t b0 = p * JPEG_BLK_PIECE, b1 = min(ubytes, b0 + JPEG_BLK_PIECE);
    const uint32_t cnt = p < npiece ? jpeg_blk_stuff<false>(words, k.stride, b0, b1, nullptr, 0u, 0u, bad) : 0u;
    const uint32_t inc = jpeg_block_scan<1024>(cnt, sbuf);
    if (t == n - 1) stot = inc;
    if (WRITE && p < npiece) jpeg_blk_stuff<true>(words, k.stride, b0, b1, a.out, dst + running + inc - cnt, k.out_size, bad);
    __syncthreads();
    running += stot;
    __syncthreads();
  }
  if (t == 0) {
    if (WRITE) {
      const uint32_t at = dst + running;
      if ((unsigned long long)at + 2ull <= (unsigned long long)k.out_size) {
        a.out[at] = 0xff;
        a.out[at + 1] = (uint8_t)(it + 1 < a.nint ? 0xD0u + (uint32_t)(it & 7) : 0xD9u);
      } else {
        bad = true;
      }
    } else {
      a.lens[gid] = running + 2u;
    }
  }
  if (bad) {
    if (WRITE) a.out[k.out_size] = 1;                // the byte behind the payload
    else atomicOr(k.err, 1u);
  }
}

}  // namespace

// Optimised tables, behind the transform: zero freq, histogram, build (fills ihuff, hdrs, hdr_lens).
static void launch_jpeg_huff_opt(const JpegArgs& a, hipStream_t s) {
  launch_zero(a.freq, (size_t)a.B * HUFF_WORDS * sizeof(uint32_t), s);
  const long long per_img = (long long)a.mx * a.my * a.nb;
  const unsigned hg = (unsigned)((per_img + HUFF_COUNT_LANES - 1) / HUFF_COUNT_LANES);
  hipLaunchKernelGGL(jpeg_huff_count_kernel, dim3(hg, (unsigned)a.B), dim3(HUFF_COUNT_LANES), 0, s, a);
  hipLaunchKernelGGL(jpeg_huff_build_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
}

// grid of a one-lane-per-item kernel: over the batch, or (optimised tables) per image with
// blockIdx.y = image
static dim3 item_grid(const JpegArgs& a, long long per_image, int lanes) {
  if (a.ihuff != nullptr) return dim3((unsigned)((per_image + lanes - 1) / lanes), (unsigned)a.B);
  return dim3((unsigned)((per_image * a.B + lanes - 1) / lanes));
}

static int blk_threads(long long items) {
  const long long t = (items + 63) / 64 * 64;
  return (int)(t < 64 ? 64 : (t > 1024 ? 1024 : t));
}

void launch_jpeg_count_blocks(const JpegArgs& a, const JpegBlkArgs& k, hipStream_t s) {
  launch_zero(k.err, 4, s);
  launch_jpeg_transform(a, s);
  if (a.ihuff != nullptr) launch_jpeg_huff_opt(a, s);
  const dim3 bg = item_grid(a, (long long)a.mx * a.my * a.nb, BLK_LANES);
  const unsigned ig = (unsigned)((long long)a.B * a.nint);
  const long long per = (long long)(a.restart < a.mx * a.my ? a.restart : a.mx * a.my) * a.nb;   // blocks per interval
  hipLaunchKernelGGL(jpeg_blk_bits_kernel, bg, dim3(BLK_LANES), 0, s, a, k);
  hipLaunchKernelGGL(jpeg_blk_scan_kernel, dim3(ig), dim3(blk_threads(per)), 0, s, a, k);
  hipLaunchKernelGGL(jpeg_blk_pack_kernel, bg, dim3(BLK_LANES), 0, s, a, k);
  // pieces per interval: sized for an eighth of the worst case, longer strings take more tiles
  const int st = blk_threads(((long long)k.stride * 4 / JPEG_BLK_PIECE + 7) / 8);
  hipLaunchKernelGGL(jpeg_blk_stuff_kernel<false>, dim3(ig), dim3(st), 0, s, a, k);
  hipLaunchKernelGGL(jpeg_scan_image_kernel, dim3(a.B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(jpeg_scan_batch_kernel, dim3(1), dim3(64), 0, s, a);
}

void launch_jpeg_write_blocks(const JpegArgs& a, const JpegBlkArgs& k, hipStream_t s) {
  launch_zero(a.out + k.out_size, 1, s);
  const unsigned ig = (unsigned)((long long)a.B * a.nint);
  const int st = blk_threads(((long long)k.stride * 4 / JPEG_BLK_PIECE + 7) / 8);
  hipLaunchKernelGGL(jpeg_blk_stuff_kernel<true>, dim3(ig), dim3(st), 0, s, a, k);
  hipLaunchKernelGGL(jpeg_header_kernel, dim3(a.B), dim3(256), 0, s, a);
}

void launch_jpeg_count(const JpegArgs& a, hipStream_t s) {
  launch_jpeg_transform(a, s);
  if (a.ihuff != nullptr) launch_jpeg_huff_opt(a, s);
  hipLaunchKernelGGL(jpeg_entropy_kernel<false>, item_grid(a, a.nint, 64), dim3(64), 0, s, a);
  hipLaunchKernelGGL(jpeg_scan_image_kernel, dim3(a.B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(jpeg_scan_batch_kernel, dim3(1), dim3(64), 0, s, a);
}

void launch_jpeg_write(const JpegArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_entropy_kernel<true>, item_grid(a, a.nint, 64), dim3(64), 0, s, a);
  hipLaunchKernelGGL(jpeg_header_kernel, dim3(a.B), dim3(256), 0, s, a);
}

void launch_jpeg_reconstruct(const JpegArgs& a, hipStream_t s) {
  const long long mcus = (long long)a.B * a.mx * a.my;
  const unsigned ig = (unsigned)((mcus + TR_WAVES - 1) / TR_WAVES);
  const unsigned cg = (unsigned)(((long long)a.B * a.H * ((a.W + 3) >> 2) + 255) / 256);
  if (a.nb == 6) {
    hipLaunchKernelGGL(jpeg_idct_kernel<true>, dim3(ig), dim3(64 * TR_WAVES), 0, s, a);
    hipLaunchKernelGGL(jpeg_colour_kernel<true>, dim3(cg), dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(jpeg_idct_kernel<false>, dim3(ig), dim3(64 * TR_WAVES), 0, s, a);
    hipLaunchKernelGGL(jpeg_colour_kernel<false>, dim3(cg), dim3(256), 0, s, a);
  }
}

void launch_jpeg_entropy_decode(const JpegArgs& a, const JpegDecodeIn& d, hipStream_t s) {
  launch_zero(a.coef, d.zero_bytes, s);
  const unsigned eg = (unsigned)(((long long)a.B * a.nint + 63) / 64);
  hipLaunchKernelGGL(jpeg_entropy_decode_kernel, dim3(eg), dim3(64), 0, s, a, d);
}

void launch_jpeg_entropy_decode_chunked(const JpegArgs& a, const JpegDecodeIn& d, const JpegSyncIn& y, int threads,
                                        hipStream_t s) {
  launch_zero(a.coef, d.zero_bytes, s);
  if (y.ngroups > 0)
    hipLaunchKernelGGL(jpeg_entropy_sync_kernel, dim3(y.ngroups), dim3(threads), 0, s, a, d, y);
  const int luma = min(a.restart, a.mx * a.my) * (a.nb - 2);
  const int dct = min(1024, (luma + 63) / 64 * 64);
  hipLaunchKernelGGL(jpeg_dc_prefix_kernel, dim3((unsigned)((long long)a.B * a.nint)), dim3(dct), 0, s, a, d, y);
  const unsigned cg = (unsigned)(((long long)a.B * a.mx * a.my * a.nb + 255) / 256);
  hipLaunchKernelGGL(jpeg_block_check_kernel, dim3(cg), dim3(256), 0, s, a, d, y);
}
