"""Command line of the burst super-resolution (the reference's run_handheld.py flags):

    python run_handheld.py --impath burst.npz --outpath out.png [--config my.yaml] [key=value ...]
    python run_handheld.py --impath burst_folder --outpath out.dng output.format=dng [output.tile=128 output.predictor=1]

--impath   a burst in an .npz file (the keys process() documents), or a folder of .dng files: where rawpy + exifread exist,
           or with the override dng.reader=native read by this package itself (handheld_super_resolution/dng.py); with
           dng.linearization=apply as well, the files' LinearizationTable, BlackLevelDeltaH / V and GainMap opcodes are
           applied on the GPU instead of being refused or ignored
--outpath  .png: 8-bit PNG;  .tif / .tiff: 16-bit uncompressed TIFF (post-processing as configured);  .dng with the override
           output.format=dng: a LinearRaw DNG of the merged linear image at 16 bits, post-processing switched off like
           upstream (whose DNG export runs exiftool and dng_validate on such a TIFF; here the file is coded on the GPU)
--config   a YAML file merged over the defaults (config.DEFAULTS)
key=value  overrides, e.g. scale=2 robustness.save_mask=false; the values are read as YAML scalars, never evaluated.  The
           optional sections of process() are reached the same way: reference.select=sharpest, noise_model.source=estimate,
           white_balance.source=estimate (white_balance.frames=2 white_balance.min_tiles=8) for a burst of integer counts
           that brings no white_balance

The image is quantised on the GPU (config.output.dtype, hhsr_encode_image) and written with the standard library
(utils_image.save_png, utils_dng.save_as_tiff).  With the override output.format=png and a .png outpath the PNG itself is
coded on the GPU (utils_image.encode_png: output.dtype uint8 | uint16, output.filter, output.interval_bytes) and the returned
bytes are written as they are; output.format=dng with a .dng outpath does the same with utils_dng.encode_dng (output.tile,
output.predictor).  With robustness.save_mask the accumulated-robustness mask goes to
<outpath stem>.rob.png like upstream."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--config", type=str, help="YAML file whose keys are merged over the built-in defaults")
    parser.add_argument("--impath", type=str, required=True, help="burst to process: an .npz file, or a folder of .dng frames")
    parser.add_argument("--outpath", type=str, required=True, help="file to write: .png (8 bits), .tif / .tiff (16 bits), or .dng with "
                                                                        "the override output.format=dng")
    parser.add_argument("overrides", nargs="*", help="dotted configuration keys set from the command line, e.g. scale=2 "
                                                     "robustness.save_mask=false (values are YAML scalars)")
    return parser.parse_args(argv)


def build_config(args):
    """Defaults, then --config, then the key=value overrides, then the output dtype the file type asks for."""
    from handheld_super_resolution.config import OmegaConf, default_config

    config = default_config()
    if args.config:
        config = OmegaConf.merge(config, OmegaConf.load(args.config))
    for item in args.overrides:
        if "=" not in item:
            raise ValueError(f"override {item!r}: expected key=value")
    if args.overrides:
        config = OmegaConf.merge(config, OmegaConf.from_dotlist(args.overrides))
    suffix = os.path.splitext(args.outpath)[1].lower()
    out_cfg = config.get("output", None) or {}
    fmt = str(out_cfg.get("format", "raw"))
    if fmt == "dng":  # process() returns the DNG file, its tiles coded on the GPU
        if suffix != ".dng":
            raise ValueError(f"output.format=dng writes a DNG file: --outpath {args.outpath!r} does not end in .dng")
        if config.postprocessing.enabled and config.verbose >= 1:
            print("output.format=dng: a DNG holds the linear image, post-processing is switched off")
        config.postprocessing.enabled = False
    elif suffix == ".dng":
        raise NotImplementedError("a .dng outpath needs the override output.format=dng (the linear image as a LinearRaw DNG, "
                                  "post-processing off); without it nothing is written: the reference's save_as_dng rewrites a "
                                  "16-bit TIFF with the external tools exiftool and dng_validate, which this build does not "
                                  "run. Or ask for .tif (the post-processed samples at 16 bits).")
    elif suffix not in (".png", ".tif", ".tiff"):
        raise ValueError(f"--outpath {args.outpath!r}: .png (8 bits), .tif / .tiff (16 bits)")
    if fmt == "png":  # output.format=png: process() returns the file, coded on the GPU
        if suffix != ".png":
            raise ValueError(f"output.format=png writes a PNG file: --outpath {args.outpath!r} does not end in .png")
    elif fmt != "dng":
        config.output = {"dtype": "uint8" if suffix == ".png" else "uint16"}
    noise = config.noise_model
    if (noise.get("alpha", None) is None) != (noise.get("beta", None) is None):
        raise ValueError("noise_model.alpha and noise_model.beta describe one noise profile: set both or neither")
    return config


def main(argv=None):
    args = parse_args(argv)
    config = build_config(args)

    from handheld_super_resolution import process
    from handheld_super_resolution.utils_dng import save_as_tiff, save_dng_bytes
    from handheld_super_resolution.utils_image import save_png, save_png_bytes

    image, debug_dict = process(args.impath, config)
    if config.verbose >= 1:
        print(f"writing {args.outpath} ({image.dtype}, {' x '.join(str(n) for n in image.shape)})")
    if image.ndim == 1 and str(config.output.get("format", "raw")) == "dng":  # the file's bytes, written as they are
        save_dng_bytes(image, args.outpath)
    elif image.ndim == 1:  # output.format=png: the file's bytes, written as they are
        save_png_bytes(image, args.outpath)
    elif image.dtype.itemsize == 1:
        save_png(image, args.outpath)
    else:
        save_as_tiff(image, args.outpath)
    if config.robustness.save_mask and debug_dict.get("robustness mask", None) is not None:
        save_png(debug_dict["robustness mask"], os.path.splitext(args.outpath)[0] + ".rob.png")
    return 0


if __name__ == "__main__":
    sys.exit(main())
