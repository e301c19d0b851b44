"""Scene for the integration check of tests/test_gpu_bsdf.py (a plain builder)."""

REFLECTANCE = (0.9, 0.8, 0.7)


def rough_floor_room(pkg, alpha, ggx, res=32):
    """mirror_room's closed room and ceiling light with a rough copper floor: roughness, distribution and specular reflectance
    reach the device through the alpha slot, the p[7] flag and rgb of the floor's BSDF record."""
    sc = pkg.scenes
    sd = sc.SceneData("rough_floor_room")
    white, red, green, black = sd.diffuse(0.725, 0.71, 0.68), sd.diffuse(0.63, 0.065, 0.05), sd.diffuse(0.14, 0.45, 0.091), sd.diffuse(0.0)
    copper = sd.roughconductor(alpha=alpha, ggx=bool(ggx), reflectance=REFLECTANCE)
    sd.rectangle(sc.translate(0, -1, 0) @ sc.rotate("x", -90), copper)
    sc._room(sd, white, red, green, walls=("ceiling", "back", "left", "right"))
    sd.rectangle(sc.translate(0, 0, 1) @ sc.rotate("y", 180), white)
    sd.rectangle(sc.translate(0, 0.995, -0.2) @ sc.rotate("x", 90) @ sc.scale(0.25), black, radiance=(17.0, 12.0, 4.0))
    sd.set_camera(sc.lookat((0, -0.2, 0.95), (0, -0.3, -0.4), (0, 1, 0)), 70.0, res, res, pkg.abi.FILTER_BOX, 0.5)
    return sd
