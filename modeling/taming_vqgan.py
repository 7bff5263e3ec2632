from maskbit_amd.taming_vqgan import OriginalVQModel  # noqa: F401
