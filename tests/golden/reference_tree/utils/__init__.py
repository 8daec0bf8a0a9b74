# the reference's utils/ is a regular package
