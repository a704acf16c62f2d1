"""The reference's ``utils`` package, by its module names: ``basic_anchors``, ``loc_bbox_iou``, ``metrics``, ``overlay`` (the demo
script's figure), ``utils`` (``update_ema``, ``ema_curve``, ``TrainingLog``) and ``draw`` (``plot_training_metrics``, ``save_png``).
Nothing is imported here: each module binds the HIP library on first use."""
