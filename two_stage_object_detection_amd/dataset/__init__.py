"""Mirror of the reference's ``dataset`` package for the input steps: reading an image file (``image_io``, the
``Image.open(path).convert("RGB")`` of ``dataset/dataloader.py``) and the transforms (``transform``, ``dataset/transform.py``)."""
