"""Replays a recorded refusal against the library under test: what test_pose_buffer_messages.py and test_compress_messages.py share. A
recording holds, per entry point, `base` -- the C arguments in order of a call that passes every check, the struct an object of its
fields that are not 0 -- and every call as its differences from them: "<index>": a C argument, "<name>": a field of the struct."""
import copy
import ctypes

from acl_amd import runtime


def struct_of(struct_type, fields, alive):
    """the ctypes struct of a recorded object; a nested object is a struct of its own, kept in `alive`, that the field points to"""
    struct = struct_type()
    for name, value in fields.items():
        if isinstance(value, dict):
            nested = struct_of(runtime.PoseBounds, value, alive)
            alive.append(nested)
            setattr(struct, name, ctypes.addressof(nested))
        elif isinstance(value, list):
            array = getattr(struct, name)
            for index, element in enumerate(value):
                array[index] = element
        else:
            setattr(struct, name, value)
    return struct


def arguments_of(base, changes):
    """the C arguments of a recorded call"""
    arguments = copy.deepcopy(base)
    struct = next(index for index, argument in enumerate(base) if isinstance(argument, dict))
    for key, value in changes.items():
        if key.isdigit():
            arguments[int(key)] = value
        else:
            arguments[struct][key] = value
    return arguments


def replay(lib, entry):
    """(status, message) of a call: entry["function"] with entry["arguments"]"""
    function = getattr(lib, entry["function"])
    alive, arguments = [], []
    for argument, argument_type in zip(entry["arguments"], function.argtypes):
        if isinstance(argument, dict):
            alive.append(struct_of(argument_type._type_, argument, alive))
            argument = ctypes.byref(alive[-1])
        arguments.append(argument)
    status = function(*arguments)
    return status, lib.aclhip_last_error_message(None).decode()
