from .unet_discriminator import UNetDiscriminatorSN  # noqa: F401
