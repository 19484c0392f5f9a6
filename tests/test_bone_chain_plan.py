"""aclhip_plan_bone_chain (host only, no device): the chain the object space single bone requests walk, root first, against a brute
force parent walk on random forests; every refusal the header lists; the NULL chain that queries the length only."""
import numpy as np
import pytest

from acl_amd import runtime

NO_PARENT = runtime.NO_PARENT


def brute_force_chain(parents, bone):
    chain = [bone]
    while chain[-1] != 0 and parents[chain[-1]] != NO_PARENT:
        chain.append(int(parents[chain[-1]]))
    return np.array(chain[::-1], dtype=np.uint32)


def random_forest(rng, num_tracks, span, extra_roots):
    parents = np.zeros(num_tracks, dtype=np.uint32)
    parents[0] = NO_PARENT
    for i in range(1, num_tracks):
        parents[i] = rng.integers(max(0, i - span), i)
    if extra_roots and num_tracks > 1:
        parents[rng.choice(np.arange(1, num_tracks), size=min(extra_roots, num_tracks - 1), replace=False)] = NO_PARENT
    return parents


@pytest.mark.parametrize("num_tracks,span,extra_roots", [(1, 1, 0), (2, 1, 0), (37, 3, 0), (100, 9, 3), (300, 40, 7), (64, 1, 5)])
def test_chain_is_the_brute_force_parent_walk(num_tracks, span, extra_roots):
    rng = np.random.default_rng(num_tracks * 31 + span)
    parents = random_forest(rng, num_tracks, span, extra_roots)
    for bone in range(num_tracks):
        expected = brute_force_chain(parents, bone)
        assert np.array_equal(runtime.plan_bone_chain(parents, bone), expected), bone
        assert runtime.plan_bone_chain(parents, bone, query_length_only=True) == expected.size
        # a capacity of exactly the chain's length is enough
        assert np.array_equal(runtime.plan_bone_chain(parents, bone, chain_capacity=expected.size), expected)


def test_a_chain_118_deep():
    parents = np.arange(-1, 118, dtype=np.int64).astype(np.uint32)      # 0xFFFFFFFF, 0, 1, ...
    chain = runtime.plan_bone_chain(parents, 118)
    assert np.array_equal(chain, np.arange(119, dtype=np.uint32))
    assert runtime.plan_bone_chain(parents, 60, query_length_only=True) == 61


def test_transform_zero_is_a_root_whatever_its_parent_index_says():
    parents = np.array([5, 0, 1, NO_PARENT, 3], dtype=np.uint32)
    assert np.array_equal(runtime.plan_bone_chain(parents, 2), [0, 1, 2])
    assert np.array_equal(runtime.plan_bone_chain(parents, 4), [3, 4])
    assert np.array_equal(runtime.plan_bone_chain(parents, 0), [0])


def test_refusals():
    parents = np.array([NO_PARENT, 0, 1, 2], dtype=np.uint32)
    # bone >= num_tracks
    for bone in (4, 5, 0xFFFFFFFF):
        with pytest.raises(runtime.AclHipError) as error:
            runtime.plan_bone_chain(parents, bone)
        assert error.value.status == runtime.ERROR_INVALID_ARGUMENT
        with pytest.raises(runtime.AclHipError):
            runtime.plan_bone_chain(parents, bone, query_length_only=True)
    # the chain does not fit
    for capacity in (0, 1, 3):
        with pytest.raises(runtime.AclHipError) as error:
            runtime.plan_bone_chain(parents, 3, chain_capacity=capacity)
        assert error.value.status == runtime.ERROR_INVALID_ARGUMENT
    # a transform precedes its parent: anywhere in the hierarchy, also off the bone's own chain
    for misplaced in (np.array([NO_PARENT, 2, 0, 1], dtype=np.uint32), np.array([NO_PARENT, 1, 0, 0], dtype=np.uint32), np.array([NO_PARENT, 0, 0, 7], dtype=np.uint32)):
        for bone in range(4):
            with pytest.raises(runtime.AclHipError) as error:
                runtime.plan_bone_chain(misplaced, bone)
            assert error.value.status == runtime.ERROR_INVALID_ARGUMENT


def test_null_arguments_through_the_c_abi():
    import ctypes
    lib = runtime.load_library()
    parents = np.array([NO_PARENT, 0, 1], dtype=np.uint32)
    length = ctypes.c_uint32(77)
    chain = np.full(3, 0xABCD, dtype=np.uint32)
    assert lib.aclhip_plan_bone_chain(None, 3, 1, chain.ctypes.data, 3, ctypes.byref(length)) == runtime.ERROR_INVALID_ARGUMENT
    assert lib.aclhip_plan_bone_chain(parents.ctypes.data, 3, 1, chain.ctypes.data, 3, None) == runtime.ERROR_INVALID_ARGUMENT
    assert lib.aclhip_plan_bone_chain(parents.ctypes.data, 0, 0, None, 0, ctypes.byref(length)) == runtime.ERROR_INVALID_ARGUMENT
    # NULL chain: the length alone, whatever the capacity says
    assert lib.aclhip_plan_bone_chain(parents.ctypes.data, 3, 2, None, 0, ctypes.byref(length)) == 0 and length.value == 3
    # a chain that is too small is not written
    assert lib.aclhip_plan_bone_chain(parents.ctypes.data, 3, 2, chain.ctypes.data, 2, ctypes.byref(length)) == runtime.ERROR_INVALID_ARGUMENT
    assert (chain == 0xABCD).all()
