"""The synthetic N-sphere generator is deterministic and in the reference schema."""
from raingun_amd.scene import Plane, Sphere
from raingun_amd.synth import SplitMix64, scene_md5, synthetic_scene, synthetic_yaml

# md5 of the YAML the benchmark's 1024-sphere scene is made from (seed 0x5EED)
SYNTH1024_MD5 = "021fa06ed673c2febd5ee6a7df1a00c3"


def test_splitmix64_reference_values():
    r = SplitMix64(0)
    # published SplitMix64 sequence for seed 0
    assert [r.next_u64() for _ in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_deterministic():
    assert synthetic_yaml(1024, 2, 5) == synthetic_yaml(1024, 2, 5)
    assert scene_md5(synthetic_yaml(1024, 2, 5)) == SYNTH1024_MD5


def test_shape():
    s = synthetic_scene(4096, 8, 8)
    assert sum(isinstance(b, Sphere) for b in s.bodies) == 4096
    assert sum(isinstance(b, Plane) for b in s.bodies) == 8
    assert s.max_recursion_depth == 8 and len(s.lights) == 3
    kinds = [b.material.surface for b in s.bodies if isinstance(b, Sphere)]
    assert 0.55 < kinds.count("Diffuse") / 4096 < 0.65
    assert 0.12 < kinds.count("Refractive") / 4096 < 0.18


def test_mixed_scene_tables_keep_the_yaml_order():
    """tests/mixed_scenes.py: the flat descriptor that rg_scene_create groups by kind holds the shuffled mix of
    kinds body for body, in YAML order.  (The grouped tables' ids live behind the scene handle; the GPU module's
    `body` layer and rg_trace tests check that they map back to these indices.)"""
    from mixed_scenes import config_scene
    from raingun_amd import _abi
    from raingun_amd.scene import AABB, Disk, SceneDesc, Texture

    s = config_scene("many")
    desc = SceneDesc(s)
    assert desc.desc.n_bodies == len(s.bodies) == 98 and desc.desc.n_textures == 2
    kind = {Sphere: _abi.BODY_SPHERE, Plane: _abi.BODY_PLANE, Disk: _abi.BODY_DISK, AABB: _abi.BODY_AABB}
    want = [kind[type(b)] for b in s.bodies]
    assert [desc.desc.bodies[i].kind for i in range(len(want))] == want
    assert len({k for k in want[:8]}) >= 3, "the first bodies are of one kind: no interleaving"
    for i, b in enumerate(s.bodies):
        p = list(desc.desc.bodies[i].p)
        head = [*b.center, b.radius] if isinstance(b, Sphere) else [*b.origin, *b.normal] if isinstance(b, Plane) \
            else [*b.origin, *b.normal, b.radius] if isinstance(b, Disk) else [*b.bounds[0], *b.bounds[1]]
        assert p[:len(head)] == head, i
        m = desc.desc.bodies[i].material
        assert (m.coloration == _abi.COLORATION_TEXTURE) == isinstance(b.material.coloration, Texture), i
        assert (m.texture >= 0) == isinstance(b.material.coloration, Texture), i
