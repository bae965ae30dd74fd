"""The rules of sk_gzip_inflate_piece_device_async (include/sickle_amd.h) stated in Python, on gunzip_model's header
parser and block-by-block inflate: piece() is one call with an ample capacity (its end, the last resume point R in front
of the first thing that does not parse inside the window, is then deterministic), stream() chains pieces over an image,
resume_points() lists every point a capacity-cut piece may end at (where it does depends on the guessed block starts and
is not pinned)."""
import struct
import zlib

import gunzip_model as gm

WINDOW = 32768
FIELDS = ("pos_bit", "in_member", "member_text", "member_crc", "members", "text_bytes")


def zero_state():
    return dict(pos_bit=0, in_member=0, member_text=0, member_crc=0, members=0, text_bytes=0, status=0, error=0, error_member=0,
                error_offset=0, done=0, mstart=0, history=bytes(WINDOW))


def piece(image, state, window_bytes, last, image_offset=0, points=None):
    """-> (state_out, text, info): info = dict(window_limited, inherited).  `image` begins at stream byte image_offset.
    points: a list that gets (stream bit, in_member) of every resume point the walk reaches."""
    st = dict(state)
    info = dict(window_limited=0, inherited=0)
    if st["status"]:
        info["inherited"] = 1
        return st, b"", info
    if st["done"]:
        return st, b"", info
    p, image_end = st["pos_bit"] >> 3, image_offset + len(image)
    if p < image_offset or p > image_end:
        st["status"] = 3
        return st, b"", info
    end = min(p + window_bytes, image_end)
    closing = bool(last) and end == image_end
    win = image[p - image_offset:end - image_offset]
    n = len(win)
    out = bytearray(st["history"])
    in_member, bit, members = st["in_member"], st["pos_bit"] & 7, 0
    floor = len(out) - st["member_text"] if in_member else 0
    crc, mlen, mstart = (st["member_crc"], st["member_text"], st["mstart"]) if in_member else (0, 0, p)
    errors, fail, ended, far_seen, first = [], None, False, False, True

    def resume():
        r = dict(bit=bit, in_member=in_member, len=len(out), members=members, crc=crc, mlen=mlen, mstart=mstart, start=first)
        if points is not None:
            points.append((8 * p + bit, in_member))
        return r

    R = resume()
    while True:
        if not in_member:
            pos = bit >> 3
            if pos == n and (closing or not first):
                ended = closing
                break
            h = gm.parse_header(win, pos)
            if h[0] != gm.OK:
                fail = (members, h[0], p + pos)
                break
            mstart, floor, crc, mlen, in_member, bit, far_seen, first = p + pos, len(out), 0, 0, 1, 8 * h[1], False, False
        r = gm.Reader(win, bit)
        while True:
            bit = r.bit
            R = resume()
            first = False
            far, before = [False], len(out)
            try:
                _, final = gm.block(r, out, floor, far)
            except gm.Bad:
                if closing and far[0] and not far_seen:
                    errors.append((members, gm.DEFLATE, p + (bit >> 3)))
                fail = (members, gm.DEFLATE, p + (bit >> 3))
                break
            if far[0] and not far_seen:
                far_seen = True
                errors.append((members, gm.DEFLATE, p + (bit >> 3)))
            crc = zlib.crc32(bytes(out[before:]), crc)
            mlen += len(out) - before
            if final:
                break
        if fail:
            break
        at = (r.bit + 7) >> 3
        if n - at < 8:
            fail = (members, gm.TRUNCATED, mstart)
            break
        want_crc, isize = struct.unpack_from("<II", win, at)
        if mlen & 0xffffffff != isize:
            errors.append((members, gm.LENGTH, mstart))
        elif crc != want_crc:
            errors.append((members, gm.CRC, mstart))
        members, in_member, bit, crc, mlen = members + 1, 0, (at + 8) * 8, 0, 0
        mstart = p + at + 8
        R = resume()
    if fail:
        if closing or R["start"]:
            errors.append(fail)
            info["window_limited"] = int(not closing)
            if not closing:
                del out[WINDOW:]
        else:
            del out[R["len"]:]
            members = R["members"]
    if errors:
        e = min(errors)
        st.update(status=1, error=e[1], error_member=st["members"] + e[0], error_offset=e[2], members=st["members"] + members)
        return st, b"", info
    text = bytes(out[WINDOW:])
    st.update(pos_bit=8 * p + R["bit"], in_member=R["in_member"], member_text=R["mlen"] if R["in_member"] else 0,
              member_crc=R["crc"] if R["in_member"] else 0, members=st["members"] + R["members"],
              text_bytes=st["text_bytes"] + len(text), done=int(ended), mstart=R["mstart"], history=bytes(out[-WINDOW:]))
    return st, text, info


def stream(image, window_bytes, grow=None):
    """Pieces over the whole image, `last` set, from the zero state until done or a failure -> (list of (state_out, text,
    info), text or None); info also tells the piece's window and whether it is a repeat.  grow: the window a
    window-limited piece is repeated with (once), else the failure ends the stream."""
    st, pieces, texts = zero_state(), [], []
    while True:
        nxt, text, info = piece(image, st, window_bytes, 1)
        info.update(window=window_bytes, stalled=0)
        if info["window_limited"] and grow:
            nxt, text, info = piece(image, st, grow, 1)
            info.update(window=grow, stalled=1)
        pieces.append((nxt, text, info))
        texts.append(text)
        if nxt["status"]:
            return pieces, None
        if nxt["done"]:
            return pieces, b"".join(texts)
        assert nxt["pos_bit"] > st["pos_bit"] or (nxt["pos_bit"] == st["pos_bit"] and nxt["in_member"] != st["in_member"])
        st = nxt


def verdict(pieces):
    """gm.gunzip's keys from a stream()'s pieces"""
    last = pieces[-1][0]
    return dict(error=last["error"], error_member=last["error_member"], error_offset=last["error_offset"], members=last["members"])


def resume_points(image):
    """every (stream bit, in_member) a piece of the valid image may end at"""
    points = []
    piece(image, zero_state(), len(image) + 1, 1, points=points)
    return set(points)
