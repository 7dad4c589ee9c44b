"""Reader of lpslam's recording stream for the tests (the writer under test is lpslam_amd/host/record.cpp).
Record = u64 type | u64 size | proto3 message of the reference's src/Serialize/SlamSerialize.proto; the field numbers are restated
below, as tests/replay_format.py restates them for writing.  `message_classes()` builds the same messages with google.protobuf from a
descriptor written out field by field (None where protobuf is absent), for the canonical-encoding check."""
import struct

CAMERA_IMAGE, SENSOR_IMU, SENSOR_GLOBAL_STATE, RESULT, SENSOR_FEATURE = 1, 2, 3, 4, 5


def read_records(path):
    """[(type, payload)] of a recording file; a truncated tail fails the assertion"""
    data = open(path, "rb").read()
    out, pos = [], 0
    while pos < len(data):
        assert pos + 16 <= len(data), "truncated record header at %d" % pos
        t, n = struct.unpack_from("<QQ", data, pos)
        assert pos + 16 + n <= len(data), "truncated payload at %d" % pos
        out.append((t, data[pos + 16:pos + 16 + n]))
        pos += 16 + n
    return out


def _varint(b, pos):
    v = shift = 0
    while True:
        c = b[pos]
        pos += 1
        v |= (c & 0x7F) << shift
        shift += 7
        if not c & 0x80:
            return v, pos


def fields(b):
    """[(field number, wire type, value)] in the order written; value: int (varint), float (64-bit), bytes (length-delimited)"""
    out, pos = [], 0
    while pos < len(b):
        key, pos = _varint(b, pos)
        num, wire = key >> 3, key & 7
        if wire == 0:
            v, pos = _varint(b, pos)
        elif wire == 1:
            v = struct.unpack_from("<d", b, pos)[0]
            pos += 8
        elif wire == 2:
            n, pos = _varint(b, pos)
            v = bytes(b[pos:pos + n])
            pos += n
        else:
            raise AssertionError("unexpected wire type %d" % wire)
        out.append((num, wire, v))
    return out


def _as_dict(b):
    d = {}
    for num, _, v in fields(b):
        assert num not in d, "field %d repeated" % num
        d[num] = v
    return d


def position(b):
    d = _as_dict(b)
    return tuple(d.get(k, 0.0) for k in (1, 2, 3)), tuple(d.get(k, 0.0) for k in (4, 5, 6))


def orientation(b):
    d = _as_dict(b)
    return tuple(d.get(k, 0.0) for k in (1, 2, 3, 4)), d.get(5, 0.0)


def global_state(b):
    d = _as_dict(b)
    p, ps = position(d[1]) if 1 in d else ((0.0,) * 3, (0.0,) * 3)
    q, qs = orientation(d[2]) if 2 in d else ((0.0,) * 4, 0.0)
    return dict(p=p, p_sigma=ps, q=q, q_sigma=qs, has_position=1 in d, has_orientation=2 in d, velocity=d.get(3), velocity_valid=bool(d.get(4, 0)))


def camera_image(payload):
    d = _as_dict(payload)
    return dict(timestamp=d.get(1, 0), data_number=d.get(2, 0), image=d.get(3, b""), odom=global_state(d[4]) if 4 in d else None,
                map=global_state(d[5]) if 5 in d else None, camera=d.get(6, 0), image_second=d.get(7), camera_second=d.get(8, 0),
                base=d.get(9), base_second=d.get(10), has_odom=bool(d.get(11, 0)), has_map=bool(d.get(12, 0)), numbers=sorted(d))


def result(payload):
    d = _as_dict(payload)
    return dict(timestamp=d.get(1, 0), state=global_state(d[2]) if 2 in d else None, numbers=sorted(d))


def message_classes():
    """{message name: class} of SlamSerialize.proto's messages written here, or None without google.protobuf"""
    try:
        from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    except ImportError:
        return None
    F = descriptor_pb2.FieldDescriptorProto
    f = descriptor_pb2.FileDescriptorProto(name="lpslam_test_SlamSerialize.proto", package="LpgfSlamSerialize", syntax="proto3")

    def msg(name, spec):
        m = f.message_type.add(name=name)
        for fname, num, typ, sub in spec:
            fd = m.field.add(name=fname, number=num, label=F.LABEL_OPTIONAL, type=typ)
            if sub:
                fd.type_name = ".LpgfSlamSerialize." + sub
    D, B, I64, I32, BY, M = F.TYPE_DOUBLE, F.TYPE_BOOL, F.TYPE_INT64, F.TYPE_INT32, F.TYPE_BYTES, F.TYPE_MESSAGE
    xyz = [("x", 1, D, None), ("y", 2, D, None), ("z", 3, D, None), ("x_sigma", 4, D, None), ("y_sigma", 5, D, None), ("z_sigma", 6, D, None)]
    msg("Position", xyz)
    msg("Velocity", xyz)
    msg("Orientation", [("w", 1, D, None), ("x", 2, D, None), ("y", 3, D, None), ("z", 4, D, None), ("sigma", 5, D, None)])
    msg("GlobalState", [("position", 1, M, "Position"), ("orientation", 2, M, "Orientation"), ("velocity", 3, M, "Velocity"),
                        ("velocityValid", 4, B, None)])
    msg("GlobalStateInTime", [("timeStamp", 1, I64, None), ("globalState", 2, M, "GlobalState")])
    msg("TrackerCoordinateSystem", [("position", 1, M, "Position"), ("orientation", 2, M, "Orientation")])
    msg("CameraImage", [("timeStamp", 1, I64, None), ("dataNumber", 2, I64, None), ("imageData", 3, BY, None), ("state_odom", 4, M, "GlobalState"),
                        ("state_map", 5, M, "GlobalState"), ("cameraNumber", 6, I32, None), ("imageData_second", 7, BY, None),
                        ("cameraNumber_second", 8, I32, None), ("imageBase", 9, M, "TrackerCoordinateSystem"),
                        ("imageBase_second", 10, M, "TrackerCoordinateSystem"), ("hasGlobalState_odom", 11, B, None), ("hasGlobalState_map", 12, B, None)])
    pool = descriptor_pool.DescriptorPool()
    fd = pool.Add(f)
    names = [m.name for m in f.message_type]
    if hasattr(message_factory, "GetMessageClass"):
        return {n: message_factory.GetMessageClass(pool.FindMessageTypeByName("LpgfSlamSerialize." + n)) for n in names}
    factory = message_factory.MessageFactory(pool)
    return {n: factory.GetPrototype(pool.FindMessageTypeByName("LpgfSlamSerialize." + n)) for n in names}


def check_canonical(records):
    """every payload parses as its message and re-serialises (deterministically) to the same bytes; False where protobuf is absent"""
    cls = message_classes()
    if cls is None:
        return False
    for t, payload in records:
        m = cls[{CAMERA_IMAGE: "CameraImage", RESULT: "GlobalStateInTime"}[t]]()
        m.ParseFromString(payload)
        assert m.SerializeToString(deterministic=True) == payload, "record type %d is not in canonical encoding" % t
    return True
