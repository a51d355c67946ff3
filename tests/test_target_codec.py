"""CPU: the optional Target key of a Request (include/minehip.h mh_message_ex): the encoder writes
the six reference keys as always and then "Target"; the _ex decoder reads it under json.Unmarshal's
rules; the old encode / decode are untouched and the old decode ignores the key."""
import ctypes

import pytest

import minehip
from minehip import _lib

U64 = (1 << 64) - 1


def encode_ex(type_, data, lower, upper, hash_, nonce, has_target, target):
    need = ctypes.c_size_t()
    minehip.lib.mh_msg_encode_ex(type_, data, len(data), lower, upper, hash_, nonce, has_target, target, None, 0,
                                 ctypes.byref(need))
    buf = ctypes.create_string_buffer(need.value)
    assert minehip.lib.mh_msg_encode_ex(type_, data, len(data), lower, upper, hash_, nonce, has_target, target, buf,
                                        need.value, ctypes.byref(need)) == minehip.MH_OK
    return buf.raw[:need.value]


def decode_ex(payload):
    mm = _lib.mh_message_ex()
    data = ctypes.create_string_buffer(len(payload) + 16)
    rc = minehip.lib.mh_msg_decode_ex(payload, len(payload), ctypes.byref(mm), data, len(payload) + 16)
    return rc, mm, data.raw[:mm.data_len]


def test_encoded_target_request_bytes():
    m = minehip.NewTargetRequest("cmu440", 0, 1_999_999, 18446744073709)
    assert m.Target == 18446744073709 and minehip.NewRequest("cmu440", 0, 9).Target is None
    assert minehip.marshal(m) == (b'{"Type":1,"Data":"cmu440","Lower":0,"Upper":1999999,"Hash":0,"Nonce":0,'
                                  b'"Target":18446744073709}')
    assert encode_ex(1, b"a<b", 3, 4, 5, 6, 1, U64) == (b'{"Type":1,"Data":"a\\u003cb","Lower":3,"Upper":4,"Hash":5,'
                                                        b'"Nonce":6,"Target":18446744073709551615}')
    assert m.String() == "[Request cmu440 0 1999999]"


def test_payload_without_target_is_the_old_encoding():
    for m in (minehip.NewJoin(), minehip.NewRequest("cmu440", 0, 9999999), minehip.NewResult(1228377698034, 1067492),
              minehip.NewRequest('a"b\\c\n<>&\x01\xff', 1, U64)):
        old = minehip.marshal(m)
        assert b"Target" not in old
        assert encode_ex(m.Type, m.Data, m.Lower, m.Upper, m.Hash, m.Nonce, 0, 12345) == old


@pytest.mark.parametrize("target", [0, 1, 18446744073709, U64])
def test_round_trip(target):
    m = minehip.NewTargetRequest("héllo <x>", 5, U64, target)
    back = minehip.unmarshal(minehip.marshal(m))
    assert back == m and back.Target == target
    rc, mm, data = decode_ex(minehip.marshal(m))
    assert rc == minehip.MH_OK and (mm.has_target, mm.reserved, mm.target) == (1, 0, target)
    assert (mm.type, mm.lower, mm.upper, data) == (1, 5, U64, m.Data)
    plain = minehip.unmarshal(minehip.marshal(minehip.NewRequest("x", 1, 2)))
    assert plain.Target is None and plain != minehip.NewTargetRequest("x", 1, 2, 0)
    rc, mm, _ = decode_ex(minehip.marshal(minehip.NewRequest("x", 1, 2)))
    assert rc == minehip.MH_OK and (mm.has_target, mm.target) == (0, 0)


def test_key_case_whitespace_and_null():
    for key in (b"target", b"TARGET", b"tArGeT"):
        m = minehip.unmarshal(b'{ "' + key + b'" : 77 , "Type":1,"Data":"x","Lower":1,"Upper":2}')
        assert m == minehip.NewTargetRequest("x", 1, 2, 77)
    # null leaves the field as it is, as for Lower: the key counts as absent
    assert minehip.unmarshal(b'{"Type":1,"Lower":null,"Target":null}') == minehip.Message(1)
    assert minehip.unmarshal(b'{"Type":1,"Target":5,"target":null}').Target == 5


@pytest.mark.parametrize("bad", [b"18446744073709551616", b"-1", b"1.5", b'"7"', b"1e3", b"01", b"true", b"[1]", b""])
def test_bad_target_is_refused_as_a_bad_lower(bad):
    for key in (b"Lower", b"Target"):
        payload = b'{"Type":1,"Data":"x","' + key + b'":' + bad + b'}'
        with pytest.raises(minehip.MinehipError) as e:
            minehip.unmarshal(payload)
        assert e.value.code == minehip.MH_EINVAL
        rc, _, _ = decode_ex(payload)
        assert rc == minehip.MH_EINVAL


def test_old_decode_ignores_the_key():
    payload = minehip.marshal(minehip.NewTargetRequest("cmu440", 3, 9, 42))
    mm = _lib.mh_message()
    data = ctypes.create_string_buffer(64)
    assert minehip.lib.mh_msg_decode(payload, len(payload), ctypes.byref(mm), data, 64) == minehip.MH_OK
    assert (mm.type, mm.lower, mm.upper, mm.hash, mm.nonce, data.raw[:mm.data_len]) == (1, 3, 9, 0, 0, b"cmu440")
    assert ctypes.sizeof(_lib.mh_message) == 48 and ctypes.sizeof(_lib.mh_message_ex) == 64


def test_abi_is_additive():
    assert minehip.lib.mh_abi_version() == 5
    for s in ("mh_msg_encode_ex", "mh_msg_decode_ex", "mh_search_first_multi", "mh_sched_submit_first",
              "mh_sched_job_target", "mh_sched_first_stats_read", "mh_server_first_stats"):
        assert s in _lib.EXPORTS
    assert ctypes.sizeof(_lib.mh_sched_stats) == 72 and ctypes.sizeof(_lib.mh_assignment) == 40
    assert ctypes.sizeof(_lib.mh_completion) == 32 and ctypes.sizeof(_lib.mh_sched_first_stats) == 32
