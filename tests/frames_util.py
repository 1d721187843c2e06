"""Tiny trees of rendered EXR frames in the reference's layout (TEST INFRASTRUCTURE ONLY), shared by the frame-bank tests:

    <root>/OpenEXR/<scene>/<scene>_<spp>_<index>_0/render_<Pass>_0001.exr       (spp = the third '_' field from the end, OpenEXRDirectory.py:20)
    <root>/tfrecords.json                                                       (the schema of TFRecordsExample.json)
"""
import json
import os

import numpy as np

from deepdenoiser_amd import openexr
from deepdenoiser_amd.render_passes import RenderPasses, _ORDERED

_FLAG = {name: "use_" + attr.lower() for attr, name in _ORDERED}


def features(passes):
    return {flag: (name in passes) for name, flag in _FLAG.items()}


def image(rng, h, w, name):
    """A random pass image as its EXR holds it: three channels, a 1-channel pass replicated (OpenEXRDirectory.py:66-68 keeps channel 0)."""
    img = rng.standard_normal((h, w, 3)).astype(np.float32)
    if RenderPasses.is_rgb_color_render_pass(name) or name == "Alpha":      # radiance is not negative (the passes go through log1p)
        img = np.abs(img)
    if RenderPasses.number_of_channels(name) == 1:
        img[...] = img[..., :1]
    return img


def write_rendering(directory, passes, h, w, rng):
    """-> {pass name: the [h, w, C] float32 array a reader must hand back}"""
    os.makedirs(directory)
    out = {}
    for name in passes:
        img = image(rng, h, w, name)
        openexr.write_image(os.path.join(directory, "render_%s_0001.exr" % name), img)
        out[name] = np.ascontiguousarray(img[..., :RenderPasses.number_of_channels(name)])
    return out


def rendering_name(scene, spp, index):
    return "%s_%d_%d_0" % (scene, spp, index)


def write_scene(root, scene, sizes_spp, source_passes, target_passes, h, w, rng, sources=2, target_spp=None):
    """One scene directory: `sources` renderings of every spp of sizes_spp with the source passes, and (target_spp) one with the target passes.
    -> {(spp, index): {pass: array}}"""
    out = {}
    for spp in sizes_spp:
        for index in range(sources):
            out[(spp, index)] = write_rendering(os.path.join(root, "OpenEXR", scene, rendering_name(scene, spp, index)), source_passes, h, w, rng)
    if target_spp is not None:
        out[(target_spp, 0)] = write_rendering(os.path.join(root, "OpenEXR", scene, rendering_name(scene, target_spp, 0)), target_passes, h, w, rng)
    return out


def write_json(root, modes, tile, spps, sources, source_passes, target_passes, target_spp="best", name="tfrecords.json"):
    """modes: {mode: [scene names]}"""
    j = {"base_exr_directory": "OpenEXR", "base_tfrecords_directory": "TFRecords",
         "modes": {m: {"group_by_samples_per_pixel": False, "tiles_height_width": tile, "examples_per_tfrecords": 16, "exr_directories": list(s)}
                   for m, s in modes.items()},
         "source": {"samples_per_pixel": list(spps), "number_of_sources_per_example": sources, "features": features(source_passes)},
         "target": {"samples_per_pixel": target_spp, "features": features(target_passes)}}
    path = os.path.join(root, name)
    with open(path, "w") as f:
        json.dump(j, f)
    return path
