"""Trainers with the reference's class names and train_step() surface: SimCLR, BYOL, BarlowTwins, DINO, SimSiam, ReLIC, MoCo, PIRL; VICReg, NNCLR, WMSE and PCL are this project's own."""
